/* hmsg_test.h -- test hooks and the benchmark's scene renderer of libhmsg.so.
 *
 * NOT part of the drop-in boundary (include/hmsg.h): nothing here replaces a reference interface.  The parity tests
 * use the hooks to pin building blocks of the path in isolation (the keep-largest DBSCAN, the stable radix sort, the
 * restated cKDTree, Python's float repr); bench.py uses hmsg_synth_render to put SURVEY 8d's synthetic stream into
 * HBM.  A host that links the library for the path itself includes hmsg.h only. */
#ifndef HMSG_TEST_H
#define HMSG_TEST_H
#include "hmsg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Benchmark utility, not part of the path: render the synthetic posed RGB-D + mask stream of SURVEY 8d
 * straight into device buffers (rgb u8 [n][H][W][3], depth u16 [n][H][W], masks u8 [n][M][H][W]);
 * mask_entity (host, i32 [n][M]) tells which scene entity each mask shows. */
int hmsg_synth_render(int32_t device_id, int32_t n_frames, int32_t H, int32_t W, int32_t M, const double* K,
                      const double* poses, const int32_t* room_of_frame, int32_t n_rooms, const double* room_boxes,
                      int32_t n_obj, const double* obj_boxes, const int32_t* room_obj_off, double depth_noise_mm,
                      uint64_t seed, uint8_t* rgb_dev, uint16_t* depth_dev, uint8_t* masks_dev, int32_t* mask_entity_host);

/* test hook: the segmented keep-largest DBSCAN (pcd_denoise_dbscan, graph_utils.py:827-880) on K caller-supplied clouds
 * (sizes[k] points each, concatenated in pts; host pointers).  core0 (optional, one byte per point): anchor hint as the
 * merge fold passes it.  out_pts (capacity = all points), out_sizes [K], out_core (core flag per kept point), out_info
 * [K][3] = changed, clusters found, contested. */
int hmsg_test_dbscan(const double* pts, int32_t K, const int64_t* sizes, double eps, int32_t min_points, const uint8_t* core0,
                     double* out_pts, int64_t* out_sizes, uint8_t* out_core, int32_t* out_info);
/* test hook: Python-repr text of n doubles, newline separated, into out[cap]; returns bytes written or -1 */
int64_t hmsg_test_format_doubles(const double* v, int64_t n, char* out, int64_t cap);

/* ---- diagnostics (tests only): the stable (key, value) radix sort every order-faithful voxel mean is built on
 * (Open3D VoxelDownSample adds points in input order; graph.py:348, generic.py:188, graph.py:456).  Host arrays,
 * sorted in place by the low key_bits bits of the key, equal keys keep their input order. */
int hmsg_test_sort_pairs(uint32_t* keys, uint64_t* vals, int64_t n, int32_t key_bits);
/* out[i] = s[i] after `len[i]` sequential float64 additions of p[i] (how Open3D accumulates a map point that many
 * pixels of a mask snapped to, generic.py:181-188), computed by the closed form the mask kernels use for long
 * repetitions. */
int hmsg_test_repeat_add(const double* s, const double* p, const int32_t* len, double* out, int64_t n);
/* host restatement of scipy.spatial.cKDTree (the reference's NN index, graph.py:362-364; used to answer bit-equal
 * nearest-neighbour ties like scipy does): index permutation after the default build (out_indices i64 [n], may be
 * NULL), node count, and query(x, k=1) answers for nq points. */
int hmsg_test_ckdtree(const double* pts, int64_t n, const double* queries, int64_t nq, int64_t* out_idx,
                      int64_t* out_indices, int64_t* out_n_nodes);

/* the C-boundary guard (csrc/hmsg_boundary.h) on a body that, by kind: 0 returns, 1 throws the library's own error
 * {HMSG_ERR_UNSUPPORTED, "x"}, 2 std::bad_alloc, 3 std::length_error("y"), 4 an int.  Returns the guard's status; the message it
 * kept is copied into msg (capacity cap).  No GPU involved. */
int hmsg_test_boundary(int32_t kind, char* msg, int64_t cap);

/* test hook: the part of hmsg_pool_instances behind the nearest-voxel step (graph.py:462-491 with feats_denoise_dbscan,
 * utils/graph_utils.py:682-728) on host arrays.  K instances; counts[k] down-sampled points of instance k, concatenated in
 * idx / valid: idx[i] is the row of table ([table_rows][dim] float32) point i snapped to, valid[i] != 0 keeps the point.
 * The kept rows are gathered with nan_to_num, clustered per instance (cosine DBSCAN, eps, min_samples) and averaged over the
 * largest cluster: out [K][dim] float32; an instance without a kept point gives zeros. */
int hmsg_test_pool_rows(int32_t device_id, int32_t K, const int32_t* counts, const int32_t* idx, const uint8_t* valid,
                        const float* table, int64_t table_rows, int32_t dim, double eps, int32_t min_samples, float* out);

/* the caching allocator's carving of a very large parked block (the frame store of a long episode handed back before the
 * merge: its block serves the merge's arenas instead of fresh hipMallocs): parks one block of `root_gb` GB, carves
 * three requests out of it, checks that they lie inside it and are disjoint, that nothing can be freed while a piece is
 * out, and that the block is whole again (same address) once every piece is back.  0 = ok, otherwise the failed check. */
int hmsg_test_allocator_carving(int32_t device_id, int32_t root_gb);

/* ONE Lloyd iteration of hmsg_kmeans / hmsg_kmeans_batch from given centres: E-step, centre sums, empty-cluster relocation,
 * averaging, shift.  X [n][dim] as it is (no centring), centers_in [k][dim]; labels [n], centers_out [k][dim], shift [k].
 * on_device 0: the host's lloyd_iter (hmsg_kmeans.hip); 1: the kernels of hmsg_kmeans_device.hip.  Random seeding practically
 * never empties a cluster, so this is how a test puts the relocation under the kernels. */
int hmsg_test_kmeans_lloyd(int32_t on_device, int32_t device_id, const float* X, int64_t n, int32_t dim, int32_t k,
                           const float* centers_in, int32_t* labels, float* centers_out, float* shift);

/* test hook: the candidate pairs of a level batch of the hierarchical merge (hmsg_set_merge_tree_batch) as its two kernels list
 * them.  boxes f64 [n][6] = AABB (min xyz, max xyz) on the host; group g = rows [group_off[g], group_off[g + 1]), group_off i64
 * [n_groups + 1] from 0 to n.  The pairs (i, j), i < j, both of one group, whose AABB IoU (bbox_iou, graph_utils.py:883-915, in
 * float64 as the host evaluates it) is > iou_thresh, ascending in (i, j): n_pairs = how many there are, the first
 * min(n_pairs, capacity) of them in pairs_out i32 [capacity][2]. */
int hmsg_test_group_pairs(int32_t device_id, int64_t n, const double* boxes, int32_t n_groups, const int64_t* group_off,
                          double iou_thresh, int32_t* pairs_out, int64_t capacity, int64_t* n_pairs);

/* test hook: the overlap counting of instance merging (find_overlapping_ratio_faiss, utils/graph_utils.py:620-662) through the
 * merge's own host code: the clouds go into a merger's point pool, get their overlap grids, and the pairs go through the same
 * work lists, launches and read-back as a fold step's.  h: a created handle -- voxel_size (radius = 1.5 * voxel_size) and
 * overlap_distance_form come from its config; it needs no map and is left as it was.
 *   K clouds of sizes[k] points, concatenated in pts (host, f64 [sum][3]).
 *   n_base ([K] or NULL): cloud k's first n_base[k] points (1 .. sizes[k]) go into its BASE grid, laid out on the box of those
 *     points alone; the points behind them into a DELTA grid on the whole cloud's box -- the grids of a cloud that has grown
 *     since it was indexed.  NULL, or n_base[k] == sizes[k]: one grid.
 *   pairs i32 [P][2]: cloud numbers, two different non-empty clouds each (anything else: HMSG_ERR_INVALID).
 *   decide_th < 0: value mode (hierarchical merge: both directions of every pair are counted); >= 0: decision mode (sequential
 *     merge: only `ratio > decide_th` matters, a direction that cannot change it may be left out).
 *   out_counts u32 [P][2]: points of the pair's SMALLER cloud (of equal sizes: the pair's first) with a point of the other cloud
 *     closer than the radius, then the same of the larger cloud (0 where that direction was not scanned).
 *   out_state u8 [P]: 0 the second direction was scanned, 1 left out because the first ratio alone exceeds decide_th, 2 decided by
 *     the box bound (fewer than decide_th * n points of the larger cloud lie near the smaller one's box).
 *   out_ratio f64 [P]: what the merge goes on with, max of the two ratios. */
int hmsg_test_overlap(hmsg_t* h, int32_t K, const int64_t* sizes, const int64_t* n_base, const double* pts, int64_t P,
                      const int32_t* pairs, double decide_th, uint32_t* out_counts, uint8_t* out_state, double* out_ratio);

/* test / measurement hook: the exhaustive overlap route of Room.merge_objects (hmsg_pair_overlaps, csrc/hmsg_objmerge.hip: every
 * point of one cloud against every point of the other) on the clouds points[off[i] .. off[i + 1]) (f64, host or device memory; off
 * i64 [n + 1] and pairs i32 [n_pairs][2] on the host): counts u32 [n_pairs][2] (host) as hmsg_cloud_set_overlaps defines them, with
 * both clouds of a pair taken from the one set.  What hmsg_cloud_set_overlaps is compared with and timed against. */
int hmsg_test_pair_overlaps(hmsg_t* h, int32_t n, const double* points, const int64_t* off, int64_t n_pairs, const int32_t* pairs,
                            double radius, uint32_t* counts);

/* test hook: what became of the object stage that hmsg_pool_instances runs beside itself for the graph begun on its scene
 * (hmsg_graph_begin registers the graph with the scene; HMSG_GRAPH_EARLY_OBJECTS=0 switches the stage off).
 *   g != NULL: the graph's own record; g == NULL: the record of the scene h, i.e. of the graph registered on it last (for a graph
 *   that is gone).  A graph that outlived its scene is asked with h == NULL.
 *   state: 0 never made -- no stage ran for the graph, hmsg_graph_finish did (or will do) all of it itself;
 *          1 consumed   -- hmsg_graph_finish took the stage's result over;
 *          2 discarded  -- the registration ended before a finish could take a result: by hmsg_reset, hmsg_destroy,
 *                          hmsg_restore_stage, hmsg_merge_tree_*, another hmsg_graph_begin on the scene or the graph's destroy
 *                          (whatever the stage had made by then is dropped, its thread joined), or the result was incomplete or
 *                          made from other instances than the scene holds at the finish;
 *          3 pending    -- the stage ran to its end beside hmsg_pool_instances and its result waits in the graph for the finish.
 *   live_threads: threads of the stage, over all scenes of the process, that were started and are not joined yet -- 0 whenever no
 *   hmsg_pool_instances call is running. */
int hmsg_test_graph_early_objects(const hmsg_graph_t* g, const hmsg_t* h, int32_t* state, int32_t* live_threads);

/* measurement hook: of the calling thread's last hmsg_sam_postprocess the labelling rounds (one read-back of the batch's "changed"
 * flags each) of the holes and of the islands pass (0: the pass did not run) and the HIP-event time of the statistics kernel's
 * launch over the logits.  Any pointer may be NULL. */
int hmsg_test_sam_post_last(int32_t* rounds_holes, int32_t* rounds_islands, double* stats_ms);
/* the labelling rounds (four scans each) of this thread's last hmsg_*nav_floor_maps call */
int hmsg_test_nav_last(int32_t* label_rounds);
/* the relaxation rounds that changed a tile and the host round trips (one read-back per batch of rounds) of this thread's last
 * hmsg_nav_clearance / hmsg_nav_distance_fields / hmsg_nav_route call.  Either pointer may be NULL. */
int hmsg_test_nav_route_last(int32_t* rounds, int32_t* round_trips);
/* the rounds (one relaxation launch per storey plus one link launch) in which a tile or a link changed, and the host round trips
 * (one read-back per batch of rounds), of this thread's last hmsg_nav_building_fields / hmsg_nav_building_route call.  Either
 * pointer may be NULL. */
int hmsg_test_nav_building_last(int32_t* rounds, int32_t* round_trips);
/* the rounds that changed a tile and the host round trips (one read-back per batch of rounds) of this thread's last
 * hmsg_nav_room_labels / hmsg_nav_room_doors call: the field's and the labels' rounds together (and the clearance's, where
 * hmsg_nav_room_doors computes one).  The doors' three read-backs are not counted.  Either pointer may be NULL. */
int hmsg_test_nav_rooms_last(int32_t* rounds, int32_t* round_trips);
/* the LDS layout of hmsg_nav_viewpoints_h's kernel (N10): force_ld 16 or 17 forces the row stride of its two bitmaps (17 only
 * where the device's limit per workgroup admits it), 0 leaves the choice to that limit; *ld_in_use is what runs then, *lds_limit
 * the limit the device reports.  Either pointer may be NULL.  The setting is the process's, not the thread's. */
int hmsg_test_nav_sight_layout(int32_t device_id, int32_t force_ld, int32_t* ld_in_use, int32_t* lds_limit);

/* measurement hook: the queries that the process's last hmsg_knn_labels call (hmsg_evaluate_semseg's included) finished by scan
 * (phase 2) -- all of them under HMSG_DEBUG_KNN_BRUTE=1. */
int64_t hmsg_test_knn_last_phase2(void);

#ifdef __cplusplus
}
#endif
#endif /* HMSG_TEST_H */
