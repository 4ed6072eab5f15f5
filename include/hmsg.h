/*
 * hmsg.h -- C ABI of the MI355X-native HMSG (Hierarchical Multi-modal Scene Graph) build + retrieval
 * path.  This is the drop-in boundary for the hot path of HorizonRobotics/HoloAgent `fsr_vln`:
 * the reference has no FFI today (its boundary is the Python class `Graph`,
 * fsr_vln/memory/hmsg/graph/graph.py:77-219); each entry point below names the reference code it
 * replaces.  INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every call returns 0 on success, <0 on error; hmsg_last_error(h) gives the message.
 *   - input pointers may be host OR device (HIP) pointers; the library detects which
 *     (hipPointerGetAttributes).  Output pointers are host pointers unless the name ends in `_dev`.
 *   - one handle = one scene = one HIP device + stream.  A handle is not thread-safe; distinct
 *     handles are independent.
 *   - all state (frames, voxel map, feature map, instances) lives in HBM and is owned by the handle.
 */
#ifndef HMSG_H
#define HMSG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hmsg_ctx hmsg_t;

enum {
    HMSG_OK = 0,
    HMSG_ERR_INVALID = -1,     /* bad argument / call order */
    HMSG_ERR_HIP = -2,         /* HIP runtime error */
    HMSG_ERR_UNSUPPORTED = -3, /* configuration outside what this build implements */
    HMSG_ERR_NOMEM = -4
};
/* What a failure inside the library becomes at this boundary (csrc/hmsg_boundary.h; no exception leaves an exported function):
 * the library's own errors keep their code and message; running out of host memory (std::bad_alloc) is HMSG_ERR_NOMEM, "out of
 * host memory"; any other C++ exception is HMSG_ERR_INVALID with its what(); anything else HMSG_ERR_INVALID, "unknown error". */

enum { HMSG_MERGE_SEQUENTIAL = 0, HMSG_MERGE_HIERARCHICAL = 1 };

/* Hydra `pipeline.*` / `main.*` keys of fsr_vln/config/semantic_scene_reconstruction_hm3d.yaml:1-39
 * that the path reads, plus the constants the reference hard-codes in graph.py (named here so the
 * oracle tests can vary them; defaults = the reference's literals). */
typedef struct hmsg_config {
    int32_t device_id;            /* HIP device ordinal */
    int32_t feat_dim;             /* CLIP_DIM (utils/constants.py:3-7): 512 / 768 / 1024 */
    int32_t height, width;        /* depth image size */
    int32_t max_frames;           /* capacity of the resident frame store */
    int32_t max_masks;            /* masks per frame upper bound (<= 256; SAM at points_per_side=12 yields <= 144) */
    double voxel_size;            /* pipeline.voxel_size */
    double depth_scale;           /* dataset scale, 1000.0 (hm3dsem.py:40, horizon.py:38) */
    double init_overlap_thresh;   /* pipeline.init_overlap_thresh */
    double overlap_thresh_factor; /* pipeline.overlap_thresh_factor */
    double iou_thresh;            /* pipeline.iou_thresh */
    double clip_masked_weight;    /* pipeline.clip_masked_weight */
    double max_mask_distance;     /* pipeline.max_mask_distance (filter_distance of create_3d_masks) */
    int32_t merge_type;           /* pipeline.merge_type: HMSG_MERGE_* */
    int32_t outlier_nb_points;    /* graph.py:355 literal 1000 */
    double outlier_radius;        /* graph.py:356 literal 1.0 */
    double pool_max_dist;         /* graph.py:460 literal 0.8 */
    double feat_dbscan_eps;       /* graph.py:484 literal 0.01 */
    int32_t feat_dbscan_min;      /* graph.py:484 literal 100 */
    double merge_dbscan_eps;      /* graph_utils.py:678 literal 0.1 */
    int32_t merge_dbscan_min;     /* graph_utils.py:678 literal 10 */
    int32_t min_instance_points;  /* graph.py:447 literal 10 */
    int32_t skip_frames;          /* pipeline.skip_frames (config/semantic_scene_reconstruction_hm3d.yaml; graph.py:339,373
                                     `range(0, len(dataset), skip_frames)`): of the frames offered to hmsg_add_frames -- counted
                                     across calls -- every skip_frames-th is kept, the others are ignored; 1 = all */
    double depth_cut;             /* dataset depth_cut in metres (dataloader/horizon.py:258-261: depth > depth_cut * scale -> 0,
                                     applied as the frames come in); 0 = none */
    double grid_resolution;       /* pipeline.grid_resolution of the room level (graph.py:942-974); 0.05 in the shipped configs */
    int32_t overlap_distance_form; /* HMSG_OVERLAP_*: which of faiss's two evaluations of the squared distance
                                     find_overlapping_ratio_faiss (utils/graph_utils.py:645-662) stands for -- see below */
} hmsg_config;

/* find_overlapping_ratio_faiss asks faiss 1.7.2 IndexFlatL2.search(k = 1) for squared float32 distances and counts D < radius**2.
 * faiss evaluates (dx*dx + dy*dy) + dz*dz per pair for fewer than 20 queries and |x|^2 + |y|^2 - 2 x.y (sgemm), clamped at 0, from
 * 20 queries on; the second form's rounding grows with |x|^2 (scenes far from the origin), and a point on the radius can land on
 * either side.  HMSG_OVERLAP_DIRECT (default): the direct form for every cloud -- what the oracle and rounds 1-4 pin.
 * HMSG_OVERLAP_FAISS_BLAS: faiss's switch -- a cloud of 20 or more points is looked up in the BLAS form, stated as
 * |p|^2 = (p0*p0 + p1*p1) + p2*p2, x.y = fma(x2, y2, fma(x1, y1, x0*y0)), dis = (|x|^2 + |y|^2) - 2*(x.y) in float32 (the order inside
 * the reference's BLAS is not ours to know); the overlap grids then reach sqrt(radius^2 + E), E the form's error bound at the
 * scene's coordinates, so no witness the form would accept is missed.  faiss itself is absent from this image:
 * oracle/hmsg_oracle.py carries the same switch, tests/test_faiss_form_switch.py compares the two. */
enum { HMSG_OVERLAP_DIRECT = 0, HMSG_OVERLAP_FAISS_BLAS = 1 };

/* Fill `cfg` with the reference defaults (hm3d yaml + graph.py literals). */
void hmsg_default_config(hmsg_config* cfg);
/* sizeof(hmsg_config) of THIS library: a binding that declares the struct itself (ctypes, cgo, JNA ...) checks its own size against it
 * before the first hmsg_default_config writes through its pointer */
size_t hmsg_config_size(void);

/* Graph.__init__ (graph.py:81-219) for the build pipeline: allocate the HBM-resident scene state. */
int hmsg_create(const hmsg_config* cfg, hmsg_t** out);
void hmsg_destroy(hmsg_t* h);
const char* hmsg_last_error(const hmsg_t* h);
const char* hmsg_version(void);

/* The library parks freed device scratch in a per-thread cache (re-allocating GBs per scene costs hundreds of
 * ms); this returns the calling thread's cached blocks to the driver. */
void hmsg_release_cached_memory(void);

/* Start a new scene on the same handle: state is cleared, the HBM allocations are kept (what a service
 * that rebuilds maps repeatedly does; the reference constructs a new Graph per scene,
 * application/semantic_scene_reconstrucion_offline/offline_mapping_create_hmsg_hm3d_benchmark.py:70-110). */
int hmsg_reset(hmsg_t* h);

/* Live kernel timing with HIP events on the handle's stream (measurement aid for bench.py): when on, the
 * heavy kernels are bracketed by event pairs; hmsg_profile_entry aggregates them per kernel name.  on = 1: the wide kernels and, in
 * the merge fold, the overlap scans and the component pass; on = 2: every phase of the fold's DBSCAN batch as well (a bracket costs
 * that chain of dependent launches ~3 us each: 35 us per fold step with all of them). */
int hmsg_set_profiling(hmsg_t* h, int32_t on);
int32_t hmsg_profile_count(hmsg_t* h);   /* distinct kernel names recorded since the last reset */
int hmsg_profile_entry(hmsg_t* h, int32_t i, char* name /*[64]*/, int64_t* launches, double* total_ms,
                       double* total_work /* algorithmic bytes, or FLOP for the MFMA kernels; may be NULL */);

/* ---- loop A of create_feature_map (graph.py:339-345): hand over posed RGB-D frames ------------
 * rgb u8 [n][H][W][3], depth u16 [n][H][W] (millimetres), pose f64 [n][16] row-major camera-to-world,
 * K f64 [9] row-major intrinsics (dataset[i] tuple contract, horizon.py:217-268). Frames are copied
 * into the handle's resident frame store; frame ids are assigned consecutively from 0. */
int hmsg_add_frames(hmsg_t* h, int32_t n, const uint8_t* rgb, const uint16_t* depth, const double* pose,
                    const double* K);

/* ---- A1+A2: create_pcd over all frames (generic.py:74-138) + voxel_down_sample + the (no-op)
 * DBSCAN + remove_radius_outlier + the NN index that replaces cKDTree (graph.py:348-364). */
int hmsg_finalize_map(hmsg_t* h);
int64_t hmsg_map_size(const hmsg_t* h);              /* V = points of the filtered global cloud */
/* nearest-neighbour queries so far (graph.py:409, :458, generic.py:181) that were bit-equal distance ties and were
 * answered by the host restatement of scipy's cKDTree traversal (statistics) */
int64_t hmsg_num_tie_queries(const hmsg_t* h);
int64_t hmsg_map_size_unfiltered(const hmsg_t* h);   /* voxels before remove_radius_outlier */
int hmsg_get_map_points(const hmsg_t* h, double* xyz /*[V][3]*/, double* rgb /*[V][3] or NULL*/);

/* ---- loop B (graph.py:373-411): per frame the encoder outputs consumed by
 * extract_feats_per_pixel's fusion math (sam_clip_feats_extractor.py:159-191):
 * masks u8 [n][M][H][W] (0/1), F_g f32 [n][D], F_masked f32 [n][M][D], F_crop f32 [n][M][D].
 * M is the row stride of this hand-over (M <= cfg.max_masks; it may differ from call to call); n_masks i32 [n]
 * (host or device, NULL = M for every frame) is the number of masks SAM actually returned for each frame:
 * rows >= n_masks[f] are padding and are ignored -- the softmax of sam_clip_feats_extractor.py:167-169 runs over
 * the frame's own masks only.  A frame with 0 masks makes the reference raise (it unpacks a 3-tuple,
 * :163-164); here such a frame contributes zero features (its touched voxels still count the frame, graph.py:411)
 * and no 3-D mask.  Frames first_frame .. first_frame+n-1 must have been added. */
int hmsg_add_frame_features(hmsg_t* h, int32_t first_frame, int32_t n, int32_t M, const uint8_t* masks,
                            const float* F_g, const float* F_masked, const float* F_crop, const int32_t* n_masks);
/* The same hand-over with the masks as SAM's UNCOMPRESSED RUN-LENGTH records (SamAutomaticMaskGenerator with
 * output_mode="uncompressed_rle": segment_anything/utils/amg.py mask_to_rle_pytorch; the generator keeps every mask in this form and
 * only expands it to bool [H][W] for output_mode="binary_mask").  No dense mask is built on either side: the records are decoded on
 * the device straight into the per-pixel membership bitsets every later stage reads.
 * The format: one mask of an H x W image is a list of counts c_0 .. c_{k-1} (k >= 1) whose sum is exactly H * W.  The image is read
 * in COLUMN-major order, position t = x * H + y; run r covers positions [S_r, S_r + c_r), S_r = c_0 + .. + c_{r-1}; even runs are
 * zeros, odd runs are ones, so a mask that starts with a one has c_0 = 0.  A zero count anywhere is an empty run.  (COCO's
 * compressed string form, output_mode="coco_rle", is not taken.)
 * masks of frames [first_frame, first_frame + n) as uncompressed RLE (format above).  n_masks i32 [n] is required;
 * T = sum n_masks; run_off i64 [T + 1] are offsets into counts (mask t of the hand-over, frames in order, masks of a
 * frame in order, owns counts[run_off[t] .. run_off[t+1])); counts u32.  M = row stride of F_masked / F_crop, as in the
 * dense call (n_masks[f] <= M <= cfg.max_masks).  Same state afterwards as hmsg_add_frame_features with the decoded masks.
 * counts, run_off, n_masks and the F arrays may be host or device pointers.
 * HMSG_ERR_INVALID, the handle unchanged (no bitset written, hmsg_last_error names the mask): run_off[0] != 0, run_off not
 * non-decreasing, a mask without counts, a mask whose counts do not sum to H * W, n_masks[f] outside [0, M]. */
int hmsg_add_frame_features_rle(hmsg_t* h, int32_t first_frame, int32_t n, int32_t M, const uint32_t* counts,
                                const int64_t* run_off, const int32_t* n_masks, const float* F_g, const float* F_masked,
                                const float* F_crop);
/* masks SAM returned for a frame (= number of 3-D masks the frame contributes) */
int32_t hmsg_get_frame_num_masks(const hmsg_t* h, int32_t frame);

/* A3+A4+A5 for every frame handed over so far: per-pixel feature fusion, NN snapping of frame and
 * mask points, last-writer-wins accumulation into the voxel feature map, 3-D mask clouds
 * (graph.py:380-415, generic.py:140-190). */
int hmsg_fuse_frames(hmsg_t* h);
int hmsg_get_map_feats(const hmsg_t* h, float* feats /*[V][D]*/, float* counter /*[V] or NULL*/);
/* The per-voxel feature sums behind hmsg_get_map_feats (graph.py:410-411): sum f32 [V][D], counter u32 [V] (host or
 * device pointers; either may be NULL on get).  Handles that fused disjoint frame windows of ONE episode (same map)
 * all-reduce them and install the result; feats = sum / counter is recomputed (graph.py:413-415).  Frame
 * contributions add commutatively, so the reduced map equals the single-handle one up to float32 summation order. */
int hmsg_get_feature_sums(const hmsg_t* h, float* sum, uint32_t* counter);
int hmsg_set_feature_sums(hmsg_t* h, const float* sum, const uint32_t* counter);
/* test/introspection: NN index of every pixel of a frame (-1 where depth == 0), i32 [H][W].  HMSG_ERR_INVALID after
 * hmsg_merge_instances on an episode whose frame store exceeded 96 GB (the merge hands that store back). */
int hmsg_get_frame_nn(const hmsg_t* h, int32_t frame, int32_t* idx);
/* test/introspection: F_p of a frame (sam_clip_feats_extractor.py:172-175), f32 [n_masks(frame)][D] */
int hmsg_get_frame_fp(const hmsg_t* h, int32_t frame, float* f_p);
/* 3-D masks of a frame (create_3d_masks): sizes i64 [n_masks(frame)] then points f64 [sum][3] */
int hmsg_get_frame_mask_sizes(const hmsg_t* h, int32_t frame, int64_t* sizes);
int hmsg_get_frame_mask_points(const hmsg_t* h, int32_t frame, double* xyz);

/* ---- A6: seq_merge / hierarchical_merge (graph_utils.py:918-1038) + small-cloud drop
 * (graph.py:445-448).
 * Threads: a handle is driven by one host thread at a time; distinct handles may be driven from distinct threads.  With
 * merge_type sequential the library itself starts ONE worker thread per handle inside hmsg_fuse_frames: seq_merge's fold
 * over the frames begins on the first frames' 3-D masks while the fusion is still producing the later ones (own HIP
 * stream, nothing shared with the caller); hmsg_merge_instances waits for it, hmsg_reset / hmsg_destroy stop it.  The
 * instances are the same either way (environment HMSG_FOLD_NOPIPE=1: no worker, the fold runs inside this call). */
int hmsg_merge_instances(hmsg_t* h);
int64_t hmsg_num_instances(const hmsg_t* h);
int hmsg_get_instance_sizes(const hmsg_t* h, int64_t* sizes /*[N]*/);
int hmsg_get_instance_points(const hmsg_t* h, double* xyz /*[sum][3], host or device*/);
int hmsg_get_instance_boxes(const hmsg_t* h, double* boxes /*[N][6]: AABB min xyz, max xyz*/);

/* ---- hierarchical_merge (graph_utils.py:989-1012) sharded over the frames of ONE episode: every handle
 * holds the whole map (all frames' geometry) but the features / masks of its own frame range only.
 *   hmsg_set_frame_window  after hmsg_finalize_map, before any feature: this handle's frames start at first_frame
 *                          (frame indices stay global; hmsg_add_frame_features continues from first_frame).
 *   hmsg_merge_tree_local  the levels of the merge tree that lie inside the window, with the thresholds the global tree
 *                          over total_frames frames has there.  first_frame must be a multiple of a power of two >= the
 *                          window length.  Leaves the unfinished list as the handle's instances (hmsg_get_instance_*),
 *                          reports the threshold of the next level, the number of lists at that level and this list's
 *                          index among them.
 *   hmsg_merge_tree_join   one cross-handle level on the handle that holds the even-indexed list: merge_3d_masks over
 *                          [mine ++ the partner's clouds] (sizes i64 [n_ext] on the host, points f64 [sum][3] on the host
 *                          or on the device -- e.g. the receive buffer of an RCCL collective) at
 *                          threshold th; final_pass != 0 also runs the last pass (threshold 0.75, :1007-1011) and the
 *                          small-cloud drop (graph.py:445-448), after which hmsg_pool_instances may follow.
 *                          n_ext == 0 with final_pass: a single handle held every frame.
 * The result is bit-identical to hmsg_merge_instances over all frames (tests/test_distributed_gloo.py). */
int hmsg_set_frame_window(hmsg_t* h, int32_t first_frame);
/* How the hierarchical merge walks a level of its tree (merge_adjacent_frames, graph_utils.py:959-986: the level's adjacent pairs
 * of lists, each through merge_3d_masks).  The pairs of a level are independent of each other:
 *    0  (default; again after hmsg_reset) one merge_3d_masks pass per pair, one after the other;
 *   >0  consecutive pairs whose input points sum to at most max_batch_points share ONE pass -- one grid build, one overlap
 *       task list, one DBSCAN batch; candidate pairs are formed inside a pair's own lists only (on the device).  A pair above
 *       the bound goes alone.  The bound limits the device memory of a pass (point pool, batch copy, grids);
 *   -1  a whole level per pass (2^31 - 1 points at most, the limit of one DBSCAN batch).
 * The instances are the same, bit for bit, whatever the value.  Honoured by hmsg_merge_instances with merge_type hierarchical
 * and by the levels hmsg_merge_tree_local plays (so by hmsg_merge_tree_sharded); hmsg_merge_tree_join is one pair and the
 * sequential merge a fold: neither is affected.  HMSG_ERR_INVALID once hmsg_merge_instances / hmsg_merge_tree_local have run
 * on the scene, for values below -1 and above 2^31 - 1. */
int hmsg_set_merge_tree_batch(hmsg_t* h, int64_t max_batch_points);
int hmsg_merge_tree_local(hmsg_t* h, int32_t total_frames, double* th_next, int64_t* lists_now, int64_t* my_index);
int hmsg_merge_tree_join(hmsg_t* h, int32_t n_ext, const int64_t* ext_sizes, const double* ext_points, double th,
                         int32_t final_pass);

/* ---- A7: per-instance feature pooling (graph.py:450-491, graph_utils.py:682-728). */
int hmsg_pool_instances(hmsg_t* h);
int hmsg_get_instance_feats(const hmsg_t* h, float* feats /*[N][D]*/);

/* ---- A11 the other way: resume from the stage artefacts.  Replaces Graph.load_full_pcd + load_full_pcd_feats +
 * load_masked_pcds_new (graph.py:3782-3990; the resume blocks of semantic_scene_reconstruction.py:114-127 and
 * offline_mapping_create_hmsg_hm3d_benchmark.py:97-107) for a host that holds the arrays: the handle is afterwards in the state
 * hmsg_pool_instances leaves it in, as far as the graph level can tell (hmsg_segment_floors / _rooms, hmsg_room_clouds,
 * hmsg_build_object_nodes, hmsg_object_views, hmsg_graph_begin / _finish / hmsg_build_graph, hmsg_save, the queries, every getter
 * of the map and the instances, hmsg_voxel_down_sample, hmsg_denoise_instances, hmsg_instance_room_share, hmsg_merge_room_objects,
 * hmsg_index_from_nodes).  Every array is host or device memory.
 *   map_xyz   f64 [V][3], V >= 1: ANY cloud -- it need not hold one point per voxel of a grid (a map written by the reference
 *             loads: Open3D's grid origin, outlier filter applied); its order is kept;
 *   map_rgb   f64 [V][3] or NULL (zeros);  map_feats f32 [V][D] or NULL (hmsg_get_map_feats then refuses), D = cfg.feat_dim;
 *   inst_off  i64 [n_inst + 1], non-decreasing from 0; inst_xyz f64 [inst_off[n_inst]][3]; inst_feats f32 [n_inst][D];
 *   K         f64 [9] row-major, the camera as hmsg_add_frames takes it.  Image width / height stay the handle's.
 * An instance of size 0 is allowed: it gets no node (the `< 10` points rule of graph.py:1611-1620) and its box is six zeros (what
 * an instance emptied by hmsg_denoise_instances has).  The boxes (hmsg_get_instance_boxes) are exact: numpy.min / max of the
 * instance's rows bit for bit, -0.0 ordered below +0.0.
 * HMSG_ERR_INVALID, the handle unchanged: the handle is not fresh (frames added, a map, a restore before: hmsg_reset first), a
 * coordinate of the map or of an instance is not finite, inst_off is not non-decreasing from 0.
 * On a restored handle hmsg_add_frames, hmsg_add_frame_features, hmsg_fuse_frames, hmsg_merge_instances, hmsg_merge_tree_local /
 * _join, hmsg_pool_instances, hmsg_get_frame_nn / _fp / _mask_sizes / _mask_points, hmsg_get_feature_sums / hmsg_set_feature_sums
 * and hmsg_allreduce_feature_sums return HMSG_ERR_INVALID ("... restored ...") without touching the device: there is no frame
 * store and no voxel bitmap behind it.  hmsg_get_map_feats has no frame counter to give.  hmsg_reset makes it a fresh handle. */
int hmsg_restore_stage(hmsg_t* h, int64_t V, const double* map_xyz, const double* map_rgb, const float* map_feats, int64_t n_inst,
                       const int64_t* inst_off, const double* inst_xyz, const float* inst_feats, const double* K);
/* The x y z of the vertex element of a binary little-endian PLY file (double or float properties; colours, normals and other
 * elements are skipped): o3d.io.read_point_cloud(path).points for full_pcd.ply and objects/pcd_<i>.ply of save_full_pcd /
 * save_masked_pcds (graph.py:3718-3780), the reader hmsg_load uses.  *n = number of vertices; xyz == NULL: the count only, else
 * HMSG_ERR_INVALID when capacity < *n.  xyz is host memory.  HMSG_ERR_INVALID for a file that cannot be opened, has no complete
 * header or fewer bytes than its header promises; HMSG_ERR_UNSUPPORTED for ascii / big-endian files and list properties of the
 * vertex element. */
int hmsg_read_ply(const char* path, double* xyz /*[capacity][3] or NULL*/, int64_t capacity, int64_t* n);

/* ---- A8: the storeys of the map -- Graph.segment_floors_manually (graph.py:624-787): the map re-sampled at 5 cm, the
 * height histogram at 1 cm (device), gaussian_filter1d(sigma = 2) on the int64 counts, find_peaks(distance = 20 bins,
 * height = 90th percentile), the 1-D DBSCAN(eps = 1 m) chaining of the peaks and the reference's pick / adjust rules
 * (numpy / scipy restated in C++ on the host: a few hundred bins), then per storey the crop of the full map by
 * y in [y_lo, y_hi] (both inclusive): point count, axis-aligned box, zero_level = lowest y in the crop, height = y_hi -
 * zero_level (:769-787).  [y_lo, y_hi] is the slab hmsg_segment_rooms / hmsg_room_clouds take.  capacity 0 asks for
 * the count only. */
typedef struct hmsg_floor {
    double y_lo, y_hi;
    double zero_level, height;
    double bbox_min[3], bbox_max[3];
    int64_t n_points;
} hmsg_floor;
int hmsg_segment_floors(hmsg_t* h, hmsg_floor* out, int32_t capacity, int32_t* n_floors);

/* ---- A8 helper: Open3D `PointCloud.voxel_down_sample(voxel_size)` of a caller-supplied cloud, output in ascending
 * (ix, iy, iz) voxel order.  Replaces `self.full_pcd.voxel_down_sample(voxel_size=0.05)` at the top of
 * segment_floors / segment_floors_manually (graph.py:496-497, 633), whose height histogram is taken over the
 * re-sampled cloud.  `points` host or device [n][3]; `out_points` host, capacity n points; *out_n = points written. */
int hmsg_voxel_down_sample(hmsg_t* h, const double* points, int64_t n, double voxel_size, double* out_points,
                           int64_t* out_n);

/* ---- A10 first step: every instance through pcd_denoise_dbscan(eps=0.05, min_points=10)
 * (graph.py:1589-1591), in place; call after hmsg_pool_instances like the reference does. */
int hmsg_denoise_instances(hmsg_t* h, double eps, int32_t min_points);

/* A10 room association (graph.py:1634-1642, find_intersection_share graph_utils.py:160-189): for every
 * instance i and room r, share[i][r] = #{room-r vertices (x,z) with an instance point within `radius` in the
 * x/z plane} / #instance points.  verts_xz f64 [sum][2] (host), vert_off i64 [n_rooms+1], share f64 [N][n_rooms]. */
int hmsg_instance_room_share(hmsg_t* h, int32_t n_rooms, const int64_t* vert_off, const double* verts_xz, double radius,
                             double* share);

/* ---- A10 + node table: segment_hmsg_objects (graph.py:1582-1736) without the per-view visibility test, which needs the
 * dataset's images and stays with the caller.  Runs the per-object pcd_denoise_dbscan(0.05, 10) if it has not run yet,
 * assigns every instance with at least 10 points to each floor whose [zero - 0.2, zero + height + 0.2] contains its
 * y-extent and, there, to the room with the largest find_intersection_share (fallback: nearest room centre), labels
 * it with the arg-max of emb . label_feats^T (identify_object, graph.py:1441-1454) and numbers it per room.  The scores are
 * float32 inputs multiplied and summed in FLOAT64 (exact products, one rounding per sum); the reference's np.dot stays in
 * float32 with BLAS's summation order, so two classes within ~1e-7 of each other could swap -- none does on the
 * reference-made fixture (every object name is compared, tests/test_objects_golden.py).  Nodes come out in the
 * reference's creation order (floors outer, instances inner).  floor_zero / floor_height f64 [n_floors];
 * room_floor i32 [n_rooms]; vert_off i64 [n_rooms + 1]; verts_xz f64 [sum][2]; label_feats f32 [n_labels][D] or NULL. */
typedef struct hmsg_node {
    int32_t instance;      /* index into the instance list (hmsg_get_instance_*) */
    int32_t floor, room;   /* room = index into the caller's room list: object id "<room_id>_<counter>" */
    int32_t counter;
    int32_t label;         /* -1 without a vocabulary */
    int64_t n_points;
} hmsg_node;
int hmsg_build_object_nodes(hmsg_t* h, int32_t n_floors, const double* floor_zero, const double* floor_height, int32_t n_rooms,
                            const int32_t* room_floor, const int64_t* vert_off, const double* verts_xz, int32_t n_labels,
                            const float* label_feats);
int64_t hmsg_num_nodes(const hmsg_t* h);
/* The view <-> object topology of segment_hmsg_objects (graph.py:1712-1734): check_object_in_view
 * (utils/graph_utils.py:95-157) for n_pairs (instance, view) pairs on the instance clouds as they are in the handle (after
 * hmsg_build_object_nodes: denoised, what the reference's mask_pcds hold at that point).  pose_inv f64 [n_views][4][4] =
 * np.linalg.inv(pose) row-major (world -> camera, computed by the caller as the reference does); wh i32 [n_views][2] = image
 * width, height; K f64 [3][3]; pair_inst / pair_view i32 [n_pairs].  visible u8 [n_pairs]: 1 when at least
 * min_visible_ratio (0.5) of ALL the cloud's points are in front of the camera and project inside the image and their
 * mean depth is <= max_depth (10.0); mean_depth f64 [n_pairs]: that mean (inf where the reference returns inf: the caller
 * picks best_view_id = the visible view of smallest mean depth, first on ties).  The two matrix products are evaluated as
 * BLAS dgemm does (one fused multiply-add chain per element, k ascending): a point seen at the image border of a frame
 * re-projects onto that border to ~1e-14, so the inside / outside decisions follow the reference only with its
 * arithmetic.  The mean is summed in a fixed device order (numpy: pairwise), equal to ~1e-16 relative. */
int hmsg_object_views(hmsg_t* h, int32_t n_views, const double* pose_inv, const int32_t* wh, const double* K, int64_t n_pairs,
                      const int32_t* pair_inst, const int32_t* pair_view, double min_visible_ratio, double max_depth,
                      uint8_t* visible, double* mean_depth);

/* ---- A9: the room clouds of segment_hmsg_room (graph.py:1086-1108).  For every room the (x, z) cell centres of its 2-D
 * region (room_xz f64 [sum][2], CSR room_off i64 [n_rooms + 1]: what map_grid_to_point_cloud returns, :1084) are
 * extruded over z_levels (np.arange(zero, zero + height, 0.05) * -1, :1088-1092), transformed by T (row-major 4x4, the
 * reference's T1: Rotation.from_euler("x", 90) as scipy gives it) and every extruded point picks its nearest neighbour
 * in the FLOOR cloud = the map points with y in [y_lo, y_hi] (full_pcd.crop, :769-775; cKDTree.query(k = 1) in the
 * reference, bit-equal ties answered by the restated cKDTree over that cloud).  A room's cloud is
 * floor_pcd.select_by_index(idx): out_index (i32, capacity out_capacity) receives, room after room, the ascending indices
 * INTO THE FLOOR CLOUD (= rank among the map points inside the slab, map order); out_sizes [n_rooms] their counts;
 * n_floor_points the size of the floor cloud.  out_index may be NULL to ask for the sizes only. */
int hmsg_room_clouds(hmsg_t* h, double y_lo, double y_hi, const double* T, int32_t n_levels, const double* z_levels,
                     int32_t n_rooms, const int64_t* room_off, const double* room_xz, int64_t* out_sizes,
                     int32_t* out_index, int64_t out_capacity, int64_t* n_floor_points);
/* The camera -> room distance table of compute_room_embeddings (utils/graph_utils.py:244-291: `np.min(cdist([pos],
 * room_points))` with pos = the camera's (x, z)) from the room clouds the last hmsg_room_clouds call left on the device -- the
 * clouds do not travel to the host and back.  q_xz f64 [n_q][2] (host), out f64 [n_q][n_rooms] (host); n_rooms is what the
 * caller sized `out` for and must be the room count of that hmsg_room_clouds call (HMSG_ERR_INVALID otherwise: a call that
 * found no floor point or failed leaves n_rooms empty rooms / no rooms, never the previous storey's).  The distance to an
 * empty room is +inf. */
int hmsg_room_camera_distances(hmsg_t* h, int32_t n_rooms, int64_t n_q, const double* q_xz, double* out);
/* ---- N1: the rooms of one storey as a label image -- segment_hmsg_room up to room_vertices (graph.py:942-1071) and
 * distance_transform (graph_utils.py:391-487), every image step a kernel (the reference: numpy + OpenCV on the host).
 * The storey's cloud is the map points with y in [y_lo, y_hi] (as hmsg_room_clouds); zero_level / height are the
 * floor's, resolution = pipeline.grid_resolution.  out_markers i32 [rows][cols] (capacity in elements; host or device
 * memory): room i is markers == i + 1 for i < n_rooms, n_rooms + 1 the outside, -1 watershed lines and the image
 * border.  map_grid_to_point_cloud (graph_utils.py:359-388) of a cell (row, col): x = (col - 10.5) * resolution +
 * xz_min[0], z = (row - 10.5) * resolution + xz_min[1].  out_markers NULL asks for rows / cols / xz_min only.
 * OpenCV is restated from its documented semantics (oracle/rooms_oracle.py says where that is not pixel-exact):
 * parity with the reference is statistical here, unlike the rest of the path. */
int hmsg_segment_rooms(hmsg_t* h, double y_lo, double y_hi, double zero_level, double height, double resolution,
                       int32_t* out_markers, int64_t capacity, int32_t* out_rows, int32_t* out_cols, int32_t* out_n_rooms,
                       double* out_xz_min);
/* nodes [hmsg_num_nodes] and/or their embeddings f32 [N][D] (either may be NULL) */
int hmsg_get_nodes(const hmsg_t* h, hmsg_node* nodes, float* embeddings);

/* ---- N2: the object level of the on-disk format written at speed.  Replaces Object.save (memory/hmsg/graph/object.py:
 * 37-57) as driven per node by save_hmsg_graph (graph.py:1801-1824): for every record <dir>/<file_stem>.ply (binary
 * little-endian double x y z of the instance cloud under the header Open3D 0.18 writes for a cloud without colours, its
 * "comment Created by Open3D" line included; the reference's objects also carry colours, which this path does not keep) and
 * <dir>/<file_stem>.json = json.dump of {"object_id", "vertices"
 * (= points[:, [0, 2]], graph.py:1715), "room_id", "name", "embedding" (pooled feature), "view_ids", "best_view_id"} in
 * that order, numbers printed like Python's float repr.  The *_json fields are JSON text supplied by the caller (a
 * quoted string, a list, null ...) and are copied verbatim.  Clouds and features are read back from HBM once;
 * n_threads host threads format and write (<= 0: one per core, at most 32). */
typedef struct {
    int32_t instance;               /* index into the instance list (hmsg_node.instance) */
    const char* file_stem;          /* str(object_id) */
    const char* object_id_json;
    const char* room_id_json;
    const char* name_json;
    const char* view_ids_json;
    const char* best_view_id_json;
} hmsg_object_record;
int hmsg_save_objects(hmsg_t* h, const char* dir, int64_t n, const hmsg_object_record* recs, int32_t n_threads);
/* N2: Room.merge_objects (fsr_vln/memory/hmsg/graph/room.py:62-129; the optional post-pass of build_hier_multimodal_scene_graph,
 * graph.py:2053-2058, `pipeline.merge_objects_graph`) for the n objects of ONE room, in room.objects order: cloud i =
 * points[off[i] .. off[i + 1]) (f64 [.][3], host or device memory), name_id[i] = any numbering of the names (equal ids = equal
 * names).  Every same-name pair i < j is tested on the device (find_overlapping_ratio_faiss(obj_i.pcd, obj_j.pcd, radius) >
 * overlap_threshold; the reference calls it with 0.01 / 0.1), then the reference's bookkeeping is followed step by step:
 * np.where order, the dictionary chaining (an object that was absorbed can still become a key), the untouched objects behind them,
 * list(set(j)) in CPython's order.  Out: n_groups groups in the order the new room.objects list has; group g = group_members[
 * group_off[g] .. group_off[g + 1]): the object that stays (and is re-numbered room_id + "_" + g) first, then the objects the
 * reference adds to it (Object.__add__, object.py:93-103), in that order.  group_off: n + 1 entries, group_members: members_capacity
 * entries (n (n + 1) always suffice: every object can become a key, a key's list holds an object once). */
int hmsg_merge_room_objects(hmsg_t* h, int32_t n, const double* points, const int64_t* off, const int32_t* name_id,
                            double overlap_threshold, double radius, int32_t* n_groups, int32_t* group_off, int32_t* group_members,
                            int32_t members_capacity);

/* ---- evaluation against ground truth (memory/hmsg/eval/hm3dsem_evaluator.py): its overlap counting and its assignment.
 * find_overlapping_ratio_faiss (utils/graph_utils.py:620-662) for pairs of clouds taken from two SETS, at any radius -- what
 * evaluate_objects asks for every predicted / ground-truth object pair whose boxes intersect (radius 0.02) and evaluate_rooms for
 * every pair of rooms (0.05).  Set A: nA clouds, cloud a = ptsA[offA[a] .. offA[a + 1]) (f64 [.][3]; offA i64 [nA + 1], starting
 * at 0, non-decreasing); set B likewise (the same arrays may be given for both).  pairs i32 [n_pairs][2] = (a, b).
 *   counts[p][0] = points of A[a] that have a point of B[b] with squared float32 distance < (float)(radius * radius),
 *   counts[p][1] = points of B[b] that have such a point of A[a];
 * the reference's ratio is max(counts[p][0] / n_a, counts[p][1] / n_b).  Points are cast to float32 as the reference casts them;
 * duplicate points count individually; an empty cloud gives 0 / 0.  Both distance forms of hmsg_config::overlap_distance_form are
 * honoured with the arithmetic stated there (in the BLAS form a cloud of 20 or more QUERY points is looked up in the expanded
 * form, |p|^2 taken once per point).  No pair is tested exhaustively: both sets are sorted once by (cloud, cell) on a lattice whose
 * cell side is the reach (widened in the BLAS form like the merge's grids), and a query point searches the 27 cells around its own
 * in the other cloud's range.  The counts are integers added with integer atomics: two calls give the same answer.
 * ptsA / ptsB / offA / offB / pairs / counts may be host or device memory.  n_pairs == 0: success, nothing is launched.
 * HMSG_ERR_INVALID with counts untouched: offsets that do not start at 0 or decrease, a pair that names no cloud, a radius that
 * is not positive.  (HMSG_ERR_INVALID after counts were zeroed: a coordinate that is not finite.) */
int hmsg_cloud_set_overlaps(hmsg_t* h, int32_t nA, const double* ptsA, const int64_t* offA, int32_t nB, const double* ptsB,
                            const int64_t* offB, int64_t n_pairs, const int32_t* pairs, double radius, uint32_t* counts);
/* The same probe with find_intersection_share's comparison (utils/graph_utils.py:160-189: cKDTree.query(k = 1,
 * distance_upper_bound = radius) on float64 points): a witness has float64 (dx*dx + dy*dy) + dz*dz < radius * radius, strict -- a
 * point at exactly the radius does not count.  find_intersection_share(map = A[a], obj = B[b]) = counts[p][0] / n_b. */
int hmsg_cloud_set_overlaps_kd(hmsg_t* h, int32_t nA, const double* ptsA, const int64_t* offA, int32_t nB, const double* ptsB,
                               const int64_t* offB, int64_t n_pairs, const int32_t* pairs, double radius, uint32_t* counts);
/* The two association matrices of evaluate_objects (hm3dsem_evaluator.py:429-458), P predicted objects (clouds, CSR) against G
 * ground-truth objects (clouds, CSR, and obb_center / obb_dims f64 [G][3]): iou[p][g] = get_3d_iou(gt box, predicted box)
 * (utils/eval_utils.py:169-200, float64), the predicted box being find_box_center_and_dims of the eight corners of the cloud's
 * axis-aligned box in Open3D's corner order (the centre is their mean added in that order, the dims their ptp; an empty cloud has
 * Open3D's box at the origin); overlap[p][g] = find_overlapping_ratio_faiss(pred, gt, radius) where iou > 0 -- through
 * hmsg_cloud_set_overlaps, the reference calls it with 0.02 -- and 0 elsewhere.  iou / overlap f64 [P][G] (either may be NULL),
 * *n_gated (optional) = pairs with iou > 0.  Arrays host or device memory.  P == 0 or G == 0: HMSG_ERR_INVALID (the reference's
 * metrics divide by zero there).  What follows in the reference -- hmsg_lsap(P, G, matrix, 1, ...) and the thresholds -- is the
 * caller's for now. */
int hmsg_eval_object_matrices(hmsg_t* h, int32_t P, const double* pred_pts, const int64_t* pred_off, int32_t G, const double* gt_pts,
                              const int64_t* gt_off, const double* gt_obb_center, const double* gt_obb_dims, double radius,
                              double* iou, double* overlap, int64_t* n_gated);
/* scipy.optimize.linear_sum_assignment(cost, maximize) restated on the host (csrc/hmsg_lsap_host.h; the solver of Crouse 2016):
 * cost f64 [nr][nc] row-major; row_ind / col_ind i32 [min(nr, nc)], rows ascending; *n_assigned = min(nr, nc).  The answer is
 * scipy's index for index, also among equally good assignments (the evaluator's matrices are mostly zeros, and its semantic
 * metrics walk every assigned pair).  HMSG_ERR_INVALID (message on stderr): NaN or -inf costs, no feasible assignment. */
int hmsg_lsap(int32_t nr, int32_t nc, const double* cost, int32_t maximize, int32_t* row_ind, int32_t* col_ind, int32_t* n_assigned);

/* The three room matrices of evaluate_rooms (hm3dsem_evaluator.py:265-341), f64 [P][G], any of which may be NULL:
 *   assoc[p][g]     = find_overlapping_ratio_faiss(pred_bev, gt_bev, radius)               (first loop nest)
 *   over_pred[p][g] = min(find_intersection_share(gt_bev, pred_bev, radius), 1)           (second loop nest)
 *   over_gt[p][g]   = min(find_intersection_share(pred_bev, gt_bev, radius), 1)
 * for the pairs behind the reference's gate, 0 elsewhere: for each ground-truth floor f in order, each ground-truth room g with
 * floor_lower[f] < gt_mean_h[g] < floor_upper[f], each predicted room p with gt_min_h[g] < pred_zero_level[p] + pred_height[p] / 2 <
 * gt_max_h[g] (all strict).  P predicted rooms: clouds in CSR form (pred_pts f64 [.][3], pred_off i64 [P + 1]); G ground-truth rooms:
 * bev clouds in CSR form; F ground-truth floors.  voxel / radius: the reference uses 0.05 / 0.05.  *n_gated (optional): cells
 * behind the gate.  Arrays host or device memory.
 * pred_bev is the predicted cloud with every y set to gt_min_h[g], then voxel_down_sample(voxel) (Open3D semantics, voxels in
 * ascending order).  Restated with the reference's quirks:
 *   - gt_room.bev_pcd is REPLACED by its own down-sample at every visit, in both nests, and down-sampling is not idempotent: the
 *     j-th visit of room g in the first nest sees vds^j(gt_g), the j-th in the second vds^(n_g + j)(gt_g), n_g = g's visits in the
 *     first nest.  A room whose mean height lies inside two floors is visited under both; the later visit overwrites the cell.
 *     (The sequence reaches a bitwise fixed point after a few rounds; versions are computed until then.)
 *   - the flattened y of a voxel of k points is (h + h + ... + h) / k added sequentially in float64, which is not h for most k;
 *     it enters both distances.
 *   - the reference writes the flattened y into the predicted graph's room cloud in place.  THIS CALL DOES NOT: pred_pts is
 *     only read.
 * HMSG_ERR_INVALID with the outputs untouched: P == 0 or G == 0, offsets that do not start at 0 or decrease, voxel or radius not
 * positive, a coordinate that is not finite.  An empty predicted (or ground-truth) cloud gives 0 in all three matrices.
 * HMSG_DEBUG_EVAL_ROOMS_PER_PAIR=1 (development) down-samples the whole flattened cloud for every pair instead of grouping every
 * predicted room once; same bits. */
int hmsg_eval_rooms(hmsg_t* h, int32_t P, const double* pred_pts, const int64_t* pred_off, const double* pred_zero_level,
                    const double* pred_height, int32_t G, const double* gt_pts, const int64_t* gt_off, const double* gt_min_h,
                    const double* gt_max_h, const double* gt_mean_h, int32_t F, const double* floor_lower, const double* floor_upper,
                    double voxel, double radius, double* assoc, double* over_pred, double* over_gt, int64_t* n_gated);

/* The ranks behind object_semantics_eval_tp_auc (hm3dsem_evaluator.py:557-589).  n assigned pairs: emb [n][D] (f32, or f64 with
 * emb_is_f64 != 0: cast to f32 first, the reference's `.float()`), the class table text [C][D] f32, class_name_id i32 [C] (equal
 * NAMES share an id: the reference compares names, not indices), target_name_id i32 [n] (the ground-truth object's category; -1:
 * not in the vocabulary).  Every row is normalised in float32 as torchmetrics' pairwise_cosine_similarity does (x / ||x||); s_c is
 * the float32 dot product of the normalised rows, summed in the kernel's own order, which does not depend on c: rows of the same
 * bits give the same similarity.  rank_t = classes c with s_c > s_t, or s_c == s_t and c > t (a stable ascending argsort read from
 * its end); rank[i] = min of rank_t over the classes t with the target's name id, C if there is none.  "Category among the k most
 * similar classes" is rank[i] < k.  A row of norm zero (embedding or class) gives NaN similarities, ordered as numpy sorts them:
 * above every number, equal among themselves -- a zero embedding ranks the classes from the table's end.
 * Arrays host or device memory.  D <= 8192.  n == 0: success, nothing is launched. */
int hmsg_eval_semantic_ranks(hmsg_t* h, int32_t n, const void* emb, int32_t emb_is_f64, int32_t D, int32_t C, const float* text,
                             const int32_t* class_name_id, const int32_t* target_name_id, int32_t* rank);

/* The evaluator's numbers in float64, in the reference's operation order (csrc/hmsg_eval_metrics_host.h; host arrays; a failed
 * call's message goes to stderr). */
typedef struct hmsg_eval_counts {
    int64_t tp, tn, fp, fn;            /* tn is 0 throughout the reference */
    double acc, prec, recall;
} hmsg_eval_counts;
/* evaluate_floors (:193-263): gt_lower / gt_upper [Fg]; pred_vertices [Fp][8][3], the bounds of a predicted floor are c_y -/+ d_y / 2
 * of find_box_center_and_dims.  Both bound lists are flattened and sorted, inner neighbours averaged pairwise; tp = positions with
 * |gt - pred| < 0.5.  HMSG_ERR_INVALID: no floors on a side, unequal counts (numpy raises in the reference). */
int hmsg_eval_floors(const double* gt_lower, const double* gt_upper, int32_t Fg, const double* pred_vertices, int32_t Fp,
                     hmsg_eval_counts* out);
/* The threshold sweep (:364-383, :467-484) of matrix M [P][G] under the assignment (row_ind, col_ind)[n]: for t in
 * np.linspace(0, 1, 11), TP = sum(M[row, col] > t), FP = P - TP, FN = G - TP; the recalls -- ONLY they -- are sorted; *ap =
 * np.trapz(precisions, sorted recalls); *acc / *prec / *recall = entry which_index of the three lists (the room dictionary reads
 * index 6; recall from the SORTED list).  Any output may be NULL. */
int hmsg_eval_metrics_from_matrix(const double* M, int32_t P, int32_t G, const int32_t* row_ind, const int32_t* col_ind, int32_t n,
                                  int32_t which_index, double* ap, double* acc, double* prec, double* recall);
/* the recount at one threshold (:497-506, instances_iou50 uses 0.5) */
int hmsg_eval_counts_at(const double* M, int32_t P, int32_t G, const int32_t* row_ind, const int32_t* col_ind, int32_t n, double threshold,
                        hmsg_eval_counts* out);
/* :343-356: mean over predicted rooms of over_pred's row maxima, mean over ground-truth rooms of over_gt's column maxima */
int hmsg_eval_hydra_means(const double* over_pred, const double* over_gt, int32_t P, int32_t G, double* hydra_prec, double* hydra_recall);
/* :585-588 from the ranks: top_k_acc[i] = (pairs with rank < top_k[i]) / n; *top_k_auc = np.trapz(accuracy at k in range(0, C, 10), k / C) */
int hmsg_eval_top_k(const int32_t* rank, int32_t n, int32_t C, const int32_t* top_k, int32_t n_top_k, double* top_k_acc, double* top_k_auc);

/* ---- the open-vocabulary semantic segmentation score of a feature map (utils/eval_utils.py, utils/metric.py; csrc/hmsg_semseg.hip).
 * text_prompt (eval_utils.py:80-95) + sim_2_label (:285-293): label_out[i] = class_label[c*], c* the smallest c with the largest
 * cosine of emb[i] against text[c].  emb [n][D] (f32, or f64 with emb_is_f64 != 0: cast to f32 first), text [C][D] f32, class_label
 * i32 [C], label_out i32 [n].  The cosine is torch's cosine_similarity in float32: every row is divided by max(||row||, 1e-8) and the
 * rows are dotted, summed in the kernel's own order, which does not depend on c: rows of the same bits give the same similarity.
 * A ZERO embedding is a real case (graph.py:479-483 pushes zeros(1, D) for an empty instance): all its similarities are 0 and it
 * gets class_label[0].  This is NOT the rule of hmsg_eval_semantic_ranks, where a zero row gives NaN similarities (torchmetrics
 * divides by the norm itself).  Arrays host or device memory.  D <= 8192.  n == 0: success, nothing is launched. */
int hmsg_semseg_instance_labels(hmsg_t* h, int32_t n, const void* emb, int32_t emb_is_f64, int32_t D, int32_t C, const float* text,
                                const int32_t* class_label, int32_t* label_out);
/* knn_interpolation (eval_utils.py:308-339; Tree_interpolation, :296-305, is k = 1): labelled points lp f64 [n][3] with lab i32 [n],
 * queries q f64 [m][3], 1 <= k <= 16.  Rows with lab == -1 are dropped first, the others keep their order (:318).  For every query
 * the k labelled rows that are smallest by (d2, index) are taken: d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in float64, uncontracted (the
 * rdist sklearn's Euclidean metric accumulates), index = the row's position after the drop.  out_label[j] i32 = the most frequent
 * label among the k, the smallest label among equally frequent ones (np.bincount(...).argmax(), :330).  out_nn_index (may be NULL)
 * i32 [m][k]: those k positions in (d2, index) order.  This is the reference's answer wherever the k-th and (k + 1)-th distance of a
 * query differ or the tied rows carry one label; AT EXACT TIES sklearn's BallTree takes whichever row its traversal met first, which
 * is no rule, and this call takes the smaller index.  The search is exact (csrc/hmsg_semseg.hip): a lattice walk per query, and a
 * scan of all rows for the queries far from every labelled row; HMSG_DEBUG_KNN_BRUTE=1 (development) scans for every query, same bits.
 * Arrays host or device memory.  HMSG_ERR_INVALID with the outputs untouched: k outside 1 .. 16 (checked first, whatever m is);
 * then m == 0 is success and nothing is launched or looked at; for m > 0: fewer than k labelled rows after the drop (sklearn raises),
 * a label below -1, a coordinate that is not finite in a query or in a labelled row that is kept (rows with lab == -1 are dropped
 * before the reference builds its tree, so what they hold does not matter here either). */
int hmsg_knn_labels(hmsg_t* h, int64_t n, const double* lp, const int32_t* lab, int64_t m, const double* q, int32_t k, int32_t* out_label,
                    int32_t* out_nn_index);
/* conf i64 [L][L], rows ground truth, columns prediction: conf[g][p] = points j with gt_label[j] == g and pred_label[j] == p, labels
 * in [0, L), L <= 4096.  Integer atomics (a histogram per workgroup in LDS while L * L counters fit, global ones otherwise): two calls
 * give the same matrix.  Arrays host or device memory.  HMSG_ERR_INVALID with conf untouched: a label outside [0, L). */
int hmsg_semseg_confusion(hmsg_t* h, int64_t m, const int32_t* gt_label, const int32_t* pred_label, int32_t L, int64_t* conf);
typedef struct hmsg_semseg_scores {
    double miou, fmiou, acc, macc;     /* mean_iou, frequency_weighted_iou, pixel_accuracy, mean_accuracy */
} hmsg_semseg_scores;
/* metric.py's numbers from the confusion matrix, float64 on the host (csrc/hmsg_eval_metrics_host.h; host arrays; a failed call's
 * message goes to stderr), quirks included: the class lists are the labels PRESENT (:212-234: the ground truth's classes, and the
 * union of ground-truth and predicted classes); mean_iou and frequency_weighted_iou skip a class absent on either side (:130, :167),
 * per_class_iou does not (:93-94 is commented out); mean_accuracy and mean_iou divide by (ground-truth classes - ignored classes
 * present in the ground truth) (:64, :139), which may be 0: the IEEE quotient is returned; frequency_weighted_iou divides by m - (the
 * ground-truth points of ignored classes) (:176) and ignores nothing else; pixel_accuracy is 0 when no counted point is left (:31-32).
 * The per-class terms are summed as np.sum sums a float64 array in ascending class order (numpy's pairwise sum), skipped classes
 * standing in it as zeros.  per_class_iou (may be NULL) f64 [L]: NaN for a class outside the union, 0 for an ignored one. */
int hmsg_semseg_metrics(const int64_t* conf, int32_t L, const int32_t* ignore, int32_t n_ignore, hmsg_semseg_scores* out,
                        double* per_class_iou);
/* The whole evaluation on a scene after hmsg_pool_instances: hmsg_semseg_instance_labels on the pooled features (cfg.feat_dim
 * columns), every instance's pool points painted with its label on the device (instances in order, duplicates kept),
 * hmsg_knn_labels of gt_pts f64 [m][3] in them, hmsg_semseg_confusion against gt_label i32 [m], hmsg_semseg_metrics.  class_label
 * and gt_label are ids in [0, L).  No instance point or feature goes to the host.  per_class_iou f64 [L] and conf i64 [L][L] may be
 * NULL; text / class_label / gt_pts / gt_label / conf host or device memory, ignore / scores / per_class_iou host.
 * HMSG_ERR_INVALID: a scene without pooled instances, and whatever the four calls refuse. */
int hmsg_evaluate_semseg(hmsg_t* h, const float* text, int32_t C, const int32_t* class_label, const double* gt_pts, const int32_t* gt_label,
                         int64_t m, int32_t k, int32_t L, const int32_t* ignore, int32_t n_ignore, hmsg_semseg_scores* scores,
                         double* per_class_iou, int64_t* conf);

/* N2, load side: the object table of a saved graph straight into a retrieval index.  For every stem <dir>/<stem>.json is
 * read and its "embedding" array parsed as float64 (object.py:75-91 load; graph.py:1892-1987 load_hmsg_graph), rows in
 * the order given; room_of_node as for hmsg_index_create (declared below).  feat_dim (optional) receives the row length.
 * HMSG_ERR_INVALID when a record is missing, has no numeric embedding (saved as "") or the lengths differ.  (Object.load
 * accepts a record saved without an embedding and leaves embedding = None; such a node cannot be scored, and skipping it
 * would shift every node index after it, so the index refuses the whole table instead.) */
struct hmsg_index;
int hmsg_index_load_objects(int32_t device_id, const char* dir, int64_t n, const char* const* stems,
                            const int32_t* room_of_node, int32_t n_threads, struct hmsg_index** out, int32_t* feat_dim);

/* ---- A9 camera -> room assignment of compute_room_embeddings (utils/graph_utils.py:244-291): out[q][s] =
 * np.min(cdist([q], set s, "euclidean")) for n_q 2-D positions (camera x/z) against n_sets 2-D point sets (room
 * clouds projected to x/z): pts_xy f64 [set_off[n_sets]][2], q_xy f64 [n_q][2], out f64 [n_q][n_sets] (inf for an empty
 * set).  Host pointers. */
int hmsg_points_min_dist_2d(int32_t device_id, int32_t n_sets, const int64_t* set_off, const double* pts_xy, int64_t n_q,
                            const double* q_xy, double* out);

/* ---- N3 (the step right before the path): LiDAR keyframe clouds -> occlusion-aware uint16 depth images.  Replaces
 * nav_agent/humble_localization_nav2/lio_mapping_loc/scripts/generate_depth.py process_frame (:612-659) per frame:
 * voxel_down_sample (:626-629), project_points (:366-396), whether_occluded_deoccfast (:125-205: z-buffer at rounded
 * pixels against a float32 buffer in point order, fb / z, cv2.dilate(rect max(1, 4 / image_scale), iterations 4),
 * np.int16, cv2.filterSpeckles(0, 1000, 1), |fb / z - disparity| >= 3) and generate_occ_depth (:399-474: last point
 * in input order wins its truncated pixel, uint16(float32(z * depth_factor))).  Host pointers.
 *   points     f64 [cloud_off[n_frames]][3]: frame f owns rows cloud_off[f] .. cloud_off[f+1]
 *   poses      f64 [n_frames][12]: world -> camera rotation (row-major 3x3) then translation; NULL: `points` are
 *              already (u, v, z) rows = generate_occ_depth's own inputs (points_image[0], points_image[1],
 *              points_camera[2]) and no projection / culling is done
 *   depth_out  u16 [n_frames][height][width]
 *   state_out  optional u8 per input point: 0 visible, 1 occluded, 2 culled by the projection; only without
 *              down-sampling (voxel_size <= 0), HMSG_ERR_INVALID otherwise
 *   stats_out  optional i64 [n_frames][4]: points after down-sampling, projected into the image, visible, depth
 *              pixels written
 *   device_ms  optional: HIP-event time of the device work (transfers excluded)
 * Down-sampled voxels are visited in ascending (ix, iy, iz) order (Open3D's order is its hash map's); a cloud whose
 * bounding box holds more than 2^37 voxels is HMSG_ERR_UNSUPPORTED. */
typedef struct {
    int32_t width, height, image_scale;
    double fx, fy, cx, cy;
    double voxel_size;      /* <= 0: no down-sampling */
    double depth_factor;    /* 1000 in the reference */
} hmsg_depth_params;
int hmsg_lidar_depth(int32_t device_id, const hmsg_depth_params* prm, int32_t n_frames, const double* points,
                     const int64_t* cloud_off, const double* poses, uint16_t* depth_out, uint8_t* state_out,
                     int64_t* stats_out, double* device_ms);

/* ---- N4 (encoder side of the path): crop_all_bounding_boxs (memory/hmsg/utils/sam_utils.py:119-147) for BOTH variants
 * the extractor asks for per frame (perception/models/sam_clip_feats_extractor.py:148-151) in one launch:
 *   out_plain[m]  = cv2.resize(crop_bbox(image, bbox[m], bbox_margin), (S, S))      (sam_utils.py:58-81, 167-183)
 *   out_masked[m] = cv2.resize(crop_image(image, mask m), (S, S))                    (:150-164, no margin)
 * image u8 [H][W][3]; segs u8 [M][H][W] (non-zero = inside; needed for out_masked); bbox f64 [M][4] XYWH (host);
 * out_* u8 [M][S][S][3] (either may be NULL); S = out_size, a multiple of 4 (512 in the reference).  image / segs /
 * out_* may be host or device pointers.  cv2.resize = INTER_LINEAR, OpenCV's 8-bit fixed-point arithmetic.  A mask whose
 * crop is empty is HMSG_ERR_INVALID (cv2.resize raises on it).  device_ms (optional): HIP-event time of the launch. */
int hmsg_crop_resize_batch(int32_t device_id, int32_t H, int32_t W, const uint8_t* image, int32_t M, const uint8_t* segs,
                           const double* bbox, double bbox_margin, int32_t out_size, uint8_t* out_plain, uint8_t* out_masked,
                           double* device_ms);

/* ---- N4b (encoder side): open_clip's inference `preprocess` on the device.  The reference sends every one of a frame's 2 M
 * crops and the frame itself through it, one PIL image at a time on the host, before the image tower
 * (utils/clip_utils.py:72-73, 88-89; called from perception/models/sam_clip_feats_extractor.py:147-158), and graph.py:1127 makes
 * the room level's per-frame view embedding through the same transform:
 *     Resize(S, BICUBIC) -> CenterCrop(S) -> ToTensor -> Normalize(mean, std)
 * What is pinned, bit for bit:
 *   - Pillow 12.2's 8-bit BICUBIC resample (ImagingResample): a horizontal pass, a uint8 image, a vertical pass; double
 *     coefficients rounded to 1 / 2^22, integer accumulation, (sum + 2^21) >> 22 clamped to 0..255; a pass whose input and
 *     output lengths are equal is skipped (a copy);
 *   - torchvision's size rules: Resize(S) makes the shorter side S and the other int(S * long / short); CenterCrop(S) starts at
 *     int(round((n - S) / 2.0)) with Python's round (halves to even);
 *   - ToTensor + Normalize in float32: ((float)u8 / 255.0f - mean[c]) / std[c], channel-first; float16 output is the
 *     round-to-nearest-even of that float32.
 * torchvision's and open_clip's composition is taken from their documented behaviour; Pillow's arithmetic is what the tests
 * check against the installed Pillow.  Coefficients are made on the host per call; the device does integer work only. */
typedef struct {
    int32_t size;       /* S: output side, 1..1024 (224) */
    int32_t out_f16;    /* 0: float32 output, else float16 */
    float mean[3];
    float std[3];       /* finite and non-zero */
} hmsg_clip_preprocess;
/* 224, float32, the OpenAI constants (0.48145466, 0.4578275, 0.40821073) / (0.26862954, 0.26130258, 0.27577711) */
void hmsg_clip_default_preprocess(hmsg_clip_preprocess* p);
/* B images of one shape, u8 [B][H][W][3] -> out [B][3][S][S] (float32, or float16 with out_f16) = preprocess(Image.fromarray(img)).
 * out_u8 (optional) u8 [B][S][S][3]: the resized and centre-cropped bytes, = np.asarray(CenterCrop(S)(Resize(S)(img))).
 * images / out / out_u8 may be host or device pointers.  B = 0 is HMSG_OK.  HMSG_ERR_INVALID (before any device work): a null
 * prm / images / out, B < 0, H or W < 1, size outside 1..1024, a non-finite mean or std, std = 0.  HMSG_ERR_UNSUPPORTED: a source
 * side above 16384, B above 65535, or a down-scale so large that the source rows of one output row do not fit the kernel's LDS.
 * device_ms (optional): HIP-event time of the launch. */
int hmsg_clip_preprocess_batch(int32_t device_id, const hmsg_clip_preprocess* prm, int32_t B, int32_t H, int32_t W,
                               const uint8_t* images, void* out, uint8_t* out_u8, double* device_ms);
/* One frame's 1 + 2 M encoder inputs in one call (sam_clip_feats_extractor.py:147-158 with clip_utils.py:72-73, 88-89):
 * out [1 + 2 M][3][S][S], row 0 the whole frame (F_g's input), rows 1..M the masked crops, rows M + 1..2 M the plain crops --
 * the order hmsg_add_frame_features takes their features in.  The crops are exactly what hmsg_crop_resize_batch(out_size =
 * crop_size, 512 in the reference) makes (same kernel), held in a scratch buffer of the call, then preprocessed like any image.
 * Arguments as in hmsg_crop_resize_batch (image, segs, out: host or device; bbox: host); crop_size a multiple of 4.  A mask with
 * an empty crop is HMSG_ERR_INVALID, as there, and like every refusal of this call it comes before anything is staged or launched.
 * device_ms (optional): HIP-event time of the three launches (the tables are made and sent up before the first event). */
int hmsg_frame_encoder_inputs(int32_t device_id, const hmsg_clip_preprocess* prm, int32_t H, int32_t W, const uint8_t* image,
                              int32_t M, const uint8_t* segs, const double* bbox, double bbox_margin, int32_t crop_size,
                              void* out, double* device_ms);
/* ---- one frame's run-length masks (the records of hmsg_add_frame_features_rle: run_off i64 [M + 1], counts u32; host or device)
 * without a handle.  Both check the records like that call and return HMSG_ERR_INVALID before anything is written.
 * handle-less: one frame's RLE masks -> membership bitsets u64 [H*W][NW], NW = ceil(max(M,1)/64), bit (i & 63) of word i >> 6
 * of pixel p (row-major p = y*W + x) = mask i covers p.  out in host or device memory.  M <= 256. */
int hmsg_rle_to_bitsets(int32_t device_id, int32_t H, int32_t W, int32_t M, const uint32_t* counts, const int64_t* run_off,
                        uint64_t* out_bits);
/* handle-less: the dense u8 [M][H][W] (0/1) masks on the device, for hmsg_crop_resize_batch / hmsg_frame_encoder_inputs,
 * so a host that holds RLE never builds or uploads a dense mask.  out_masks in host or device memory. */
int hmsg_rle_to_masks(int32_t device_id, int32_t H, int32_t W, int32_t M, const uint32_t* counts, const int64_t* run_off,
                      uint8_t* out_masks);

/* ---- SAM's mask post-processing: the decoder's logits of one frame -> those records, made on the device.  Everything
 * SamAutomaticMaskGenerator.generate does behind predict_torch for crop_n_layers = 0 (segment_anything/
 * automatic_mask_generator.py: _process_batch, postprocess_small_regions; the reference hands its models.sam.* keys to it in
 * graph.py:191-199 and calls it in sam_clip_feats_extractor.py:117).  Handle-less; runs on a stream of its own.
 * Every threshold is a float32 and compared in float32, as torch compares a float32 tensor with a Python number.
 *   1. keep iou_preds[i] > pred_iou_thresh (skipped when the threshold is <= 0);
 *   2. calculate_stability_score (utils/amg.py): I = #{logit > mask_threshold + offset}, U = #{logit > mask_threshold - offset},
 *      both thresholds formed in float32, score = float32(I) / float32(U); keep score >= stability_score_thresh (U = 0: NaN,
 *      dropped; skipped when the threshold is <= 0);
 *   3. mask = logit > mask_threshold; batched_mask_to_box: XYXY = the inclusive extremes of the set pixels, [0, 0, 0, 0] for an
 *      empty mask.  With one crop equal to the image is_box_near_crop_edge removes nothing: there is no such filter here;
 *   4. torchvision.ops.nms on the float32 boxes with scores iou_preds: boxes visited by decreasing score, a visited box that is
 *      not suppressed is kept and suppresses every later box with inter / (a_i + a_j - inter) > box_nms_thresh, a = (x2 - x1) *
 *      (y2 - y1) without + 1, inter the product of the clamped overlaps, all float32, 0 / 0 = NaN suppresses nothing;
 *   5. min_mask_region_area > 0 only -- postprocess_small_regions: every kept mask, in that order, through remove_small_regions
 *      (utils/amg.py) in mode "holes" (8-connected components of the complement; every one of fewer than `area` pixels becomes
 *      foreground, border components too) and then "islands" (8-connected components of the result; if one is smaller than
 *      `area`, only those of at least `area` pixels stay, or the largest when there is none).  A mask in which neither mode
 *      found a small component scores 1.0, else 0.0; boxes are re-made from the new masks; a second NMS with these scores
 *      and box_nms_thresh; a kept mask of score 0.0 takes its new pixels and box;
 *   6. out, in the order the last NMS left: counts / run_off = the records of hmsg_add_frame_features_rle (column-major, a leading
 *      0 when pixel (0, 0) is set), area = the sum of the odd runs, bbox_xywh = box_xyxy_to_xywh = [x1, y1, x2 - x1, y2 - y1] (one
 *      less than the pixel extent: what mask["bbox"] holds and hmsg_crop_resize_batch is given in the reference),
 *      stability_score and keep_idx (the row of `logits`) of the original mask.
 * This library's own definitions, where the published sources leave a point open or nothing installed here can pin it:
 *   - among equal NMS scores the lower position goes first (a stable sort; torch's order among ties is unspecified, and the
 *     second NMS is all ties);
 *   - among equally large components in the "largest component" case the one whose first pixel comes first in row-major order
 *     wins (scipy.ndimage.label's numbering; OpenCV's is believed to be the same, unverified);
 *   - scalar thresholds are rounded to float32.
 * Pointers other than n_out and n_counts may be host or device memory.  Errors come before anything is written to the caller's
 * arrays: HMSG_ERR_INVALID for a null prm / logits / iou_preds / n_out / run_off / counts, N < 0, H or W < 1, max_out < 0, a
 * non-finite parameter, a negative area; HMSG_ERR_UNSUPPORTED for H * W >= 2^24 (the float32 counts would stop being exact).
 * N = 0 is HMSG_OK with n_out = 0 and run_off[0] = 0.  More than max_out surviving masks, or more than counts_cap counts:
 * HMSG_ERR_INVALID, only n_out and n_counts are written and hold what is needed (the message, on stderr like every handle-less
 * call's, names both): call again with larger arrays.  device_ms (optional): HIP-event time from the first launch to the last.
 * Out of scope: crop_n_layers > 0 (the crop-edge filter, the cross-crop NMS), the decoder's own up-sampling of its 256 x 256
 * logits, float16 logits, COCO's compressed strings, the unused filter_masks of utils/sam_utils.py. */
typedef struct {
    float   pred_iou_thresh;        /* 0.88 */
    float   stability_score_thresh; /* 0.95 */
    float   stability_score_offset; /* 1.0  */
    float   mask_threshold;         /* 0.0  (Sam.mask_threshold) */
    float   box_nms_thresh;         /* 0.7  */
    int32_t min_mask_region_area;   /* 0 = off (SAM's default); 100 in every config of the reference */
} hmsg_sam_post_params;
void hmsg_sam_post_default_params(hmsg_sam_post_params* p);   /* the values above, area 0 */
int hmsg_sam_postprocess(int32_t device_id, const hmsg_sam_post_params* prm,
                         int32_t N, int32_t H, int32_t W,
                         const float* logits,      /* f32 [N][H][W]: predict_torch(..., return_logits=True), flattened over (prompt, 3) */
                         const float* iou_preds,   /* f32 [N] */
                         int32_t max_out, int64_t counts_cap,
                         int32_t* n_out,           /* host */
                         int64_t* n_counts,        /* host: counts written (or needed, see errors) */
                         int32_t* keep_idx,        /* i32 [max_out]: row of `logits` each output mask came from */
                         uint32_t* counts, int64_t* run_off /* [max_out + 1] */,
                         double* bbox_xywh,        /* f64 [max_out][4], what hmsg_crop_resize_batch takes as `bbox` */
                         int32_t* area, float* stability_score,   /* [max_out] */
                         uint8_t* out_masks,       /* optional u8 [max_out][H][W], 0/1 */
                         double* device_ms);

/* ---- A11: the other node records of save_hmsg_graph (graph.py:1801-1824) -- floors/<f>.{ply,json} (floor.py:37-52),
 * rooms/<f>_<r>.{ply,json} (room.py:309-337), views/<id>.json (view.py:56-74) -- from a C / C++ host, byte for byte what
 * json.dump writes: one JSON object per call, fields in the order given (the reference's key order).  A field is either RAW
 * (value_json: the caller's JSON text for strings, id lists, null ...) or numbers the library prints like Python does
 * (float.__repr__ of the double for F64 / F32, decimal integers for I64): a scalar (ndim 0), [n0] (ndim 1) or [n0][n1]
 * (ndim 2; n0 = 0 gives []).  hmsg_write_ply writes a cloud as Open3D's write_point_cloud does (x y z doubles);
 * hmsg_read_json_numbers reads the numbers of one key back, flattened, as json.load + np.array would see them. */
enum { HMSG_JSON_RAW = 0, HMSG_JSON_F64 = 1, HMSG_JSON_F32 = 2, HMSG_JSON_I64 = 3 };
typedef struct hmsg_json_field {
    const char* key;          /* written between quotes as it is */
    int32_t kind;             /* HMSG_JSON_* */
    int32_t ndim;             /* 0, 1, 2 (numbers only) */
    int64_t n0, n1;
    const void* data;         /* RAW: const char* JSON text;  numbers: host array */
} hmsg_json_field;
int hmsg_write_json(const char* path, int32_t n_fields, const hmsg_json_field* fields);
int hmsg_write_ply(const char* path, const double* xyz, int64_t n);
int hmsg_read_json_numbers(const char* path, const char* key, double* out, int64_t capacity, int64_t* n);

/* ---- A9 / A11 bookkeeping for a C / C++ host (host arrays in, host arrays out; no device work).
 *
 * hmsg_assign_cameras_to_rooms -- compute_room_embeddings' camera -> room step (utils/graph_utils.py:257-291): camera i, if its
 * height cam_height[i] lies inside [y_min, y_max] (the floor cloud's bounds), goes to the room with the smallest
 * dist[i * n_rooms + r] (hmsg_room_camera_distances / hmsg_min_dist_2d; first minimum, as np.argmin); a room that got no camera
 * takes the closest camera OUTSIDE the bounds (sic; camera 0 when there is none, as np.argmin over a table of inf).
 * room_of_cam[n_cams]: the room of every camera inside the bounds, -1 for the others.  The rooms' image lists come back as
 * a CSR table: room_off[n_rooms + 1], room_imgs[room_off[r] .. room_off[r + 1]) in ascending camera order (capacity
 * n_cams + n_rooms entries).
 *
 * hmsg_pick_representative_views -- what follows KMeans in compute_room_embeddings (:334-352): for every label that occurs
 * (ascending, as np.unique), the member whose embedding has the largest dot product with its cluster centre (first maximum).
 * The KMeans fit itself stays on the host side of the boundary: the reference calls scikit-learn's
 * KMeans(n_clusters = num_views, n_init = 5, max_iter = 100, random_state = 0) and so does holoagent_amd/graph.py; a C host brings
 * labels and centres from whatever KMeans it links.  embs [n x D] and centers [k x D] are float32; the products are accumulated
 * in float64.  (A cluster of two members is an exact tie -- both are equally far from their mean -- which the reference
 * decides by float32 rounding inside np.dot; there, and only there, the pick may be the other member.)
 * out_member[<= k]: indices into the room's image list, one per label present; *n_out their number.
 *
 * hmsg_graph_edges -- create_graph_new (graph.py:1752-1775) as an edge list.  Node ids: 0 = the building, then the floors,
 * the rooms (in the order of room_floor), the objects, the views.  Edges in the reference's insertion order: per floor
 * (0, floor); per room of the floor (floor, room); per object of the room, ascending (room, object); then per view
 * (room, view) if view_room[v] >= 0 (a freshly built graph has none: graph.py:1176-1189 compares a string id with an int),
 * and (view, object) for its objects view_obj[view_obj_off[v] .. view_obj_off[v + 1]) in ascending object order, each once.
 * edges: capacity pairs of int64; *n_edges is set even when the capacity is too small (HMSG_ERR_INVALID then). */
/* hmsg_kmeans -- the fit between the two calls above (utils/graph_utils.py:329-333:
 * `KMeans(n_clusters=num_views, max_iter=100, n_init=5, random_state=0).fit(room_clip_embeddings)`), for a host without
 * scikit-learn.  X f32 [n][dim] (n >= k); labels i32 [n], centers f32 [k][dim] = labels_ / cluster_centers_; inertia, n_iter
 * optional.  A restatement of scikit-learn 1.7.2's Lloyd KMeans with k-means++ seeding under numpy's RandomState(seed)
 * (holoagent_amd/csrc/hmsg_kmeans.hip says statement by statement what it follows, and which three BLAS / einsum sums are
 * accumulated in float64 here because their order is the library's own: a point whose two nearest centres tie to ~1e-7
 * relative may be labelled differently).  tests/test_kmeans_cabi.py holds it to scikit-learn itself. */
int hmsg_kmeans(const float* X, int64_t n, int32_t dim, int32_t k, int32_t n_init, int32_t max_iter, uint32_t seed,
                int32_t* labels, float* centers, float* inertia, int32_t* n_iter);
/* hmsg_kmeans_batch -- hmsg_kmeans for n_sets independent problems in one call, on the device (holoagent_amd/csrc/
 * hmsg_kmeans_device.hip).  Set s is the rows set_off[s] .. set_off[s + 1] of X (set_off on the host, set_off[0] = 0); labels
 * [set_off[n_sets]], centers [n_sets][k][dim], inertia / n_iter [n_sets] (optional).  X, labels, centers, inertia and n_iter may
 * each be host or device memory.  The result equals hmsg_kmeans called once per set with the same arguments BIT FOR BIT: every
 * float32 sum keeps its order and every float64 sum of float32 products the host's eight running sums, so both differ from
 * the libraries scikit-learn calls in the same three places (the sgemm of the E-step, the einsum of the centre norms and the
 * sgemv / dgemm of the k-means++ potentials are accumulated in float64 and rounded once).  All n_sets * n_init fits run side by
 * side; no host round trip per Lloyd iteration or per chosen centre.  Argument rules are hmsg_kmeans', set by set: a set with
 * fewer than k rows (or none) makes the call return HMSG_ERR_INVALID before anything is written; n_sets = 0 is HMSG_OK and touches
 * nothing.  dim above 12288: HMSG_ERR_UNSUPPORTED.  Runs on a stream of its own and returns when the outputs are complete. */
int hmsg_kmeans_batch(int32_t device_id, int32_t n_sets, const int64_t* set_off, const float* X, int32_t dim, int32_t k,
                      int32_t n_init, int32_t max_iter, uint32_t seed, int32_t* labels, float* centers, float* inertia,
                      int32_t* n_iter);
int hmsg_assign_cameras_to_rooms(const double* dist, int64_t n_cams, int32_t n_rooms, const double* cam_height, double y_min,
                                 double y_max, int32_t* room_of_cam, int64_t* room_off, int32_t* room_imgs);
int hmsg_pick_representative_views(const float* embs, int64_t n, int32_t dim, const int32_t* labels, const float* centers,
                                   int32_t k, int32_t* out_member, int32_t* n_out);
int hmsg_graph_edges(int32_t n_floors, int32_t n_rooms, const int32_t* room_floor, int32_t n_objects, const int32_t* obj_room,
                     int32_t n_views, const int32_t* view_room, const int64_t* view_obj_off, const int32_t* view_obj,
                     int64_t* edges, int64_t capacity, int64_t* n_edges);

/* ---- (b) the graph as ONE object behind the boundary: build_hier_multimodal_scene_graph (graph.py:2033-2076), save_hmsg_graph
 * (:1801-1824) and load_hmsg_graph (:1892-1987) without a line of host bookkeeping on the caller's side.  A C / C++ host builds,
 * saves, loads and queries with four calls (tests/host_c/hmsg_host.c); holoagent_amd/graph.py's Graph keeps the reference's method
 * names on top of the same object.
 *
 *   hmsg_build_graph   after hmsg_pool_instances: segment_floors_manually (:624-787) -> per storey segment_hmsg_room (:920-1189:
 *       regions by the device watershed, room clouds, camera -> room assignment, KMeans(num_views) representative views
 *       (hmsg_kmeans), Room and View nodes with the reference's ids: rooms "<floor>_<i>", views "<floor>_<i>_<k>" with k
 *       counting across the storey's rooms, View.room_id the per-floor room INDEX) -> segment_hmsg_objects (:1582-1736: objects
 *       "<room_id>_<counter>", names from the label vocabulary, view_ids / best_view_id by check_object_in_view on the device)
 *       -> create_graph_new (:1752-1775).
 *         poses       f64 [n_frames][16] camera -> world of the PROCESSED frames (frame i of this table = dataset image
 *                     i * skip_frames), row-major;
 *         poses_inv   their np.linalg.inv, or NULL: computed here by LU with partial pivoting (a LAPACK build that orders the
 *                     eliminations differently can differ in the last bit, and a point on an image border decides by it);
 *         view_feats  f32 [n_frames][D]: the frames' global CLIP features (the F_g of loop B; graph.py:1119-1130 recomputes them);
 *         img_paths   optional, [n_frames]: dataset.frameId2imgPath of those frames (View.img_path);
 *         label_feats f32 [n_labels][D] + label_names [n_labels] (get_label_feats), or 0 / NULL: every object is "object".
 *   hmsg_graph_begin / hmsg_graph_finish   the same in two halves, so that the room level runs BESIDE the fusion and the merge
 *       fold: begin right after hmsg_finalize_map (floors, regions, room clouds and the camera table on the device, then the
 *       KMeans fits on host threads, or with hmsg_graph_params::kmeans_device on the device), finish after hmsg_pool_instances
 *       (joins them; views, objects, edges).
 *   hmsg_save   the whole directory in the reference layout: <dir>/floors/<f>.{ply,json}, rooms/<f>_<r>.{ply,json},
 *       objects/<id>.{ply,json}, views/<id>.json -- byte for byte what the mirror's Floor / Room / Object / View .save() write
 *       (tests/test_scene_graph_cabi.py), which tests/golden/persist.json pins to the reference's own classes.
 *   hmsg_load   the same directory back: nodes in the loader's order (sorted file names: rooms and objects lexicographic),
 *       object embeddings as float64, Room - View edges by id.  The result is a graph without a scene handle.
 *   hmsg_graph_index / hmsg_graph_query   the retrieval index with the upper levels resident (floors -> rooms, view
 *       embeddings, room_key = int(room_id.split("_")[-1]); room_name_emb f64 [rooms][D]: the CLIP embeddings of the rooms' names,
 *       NULL = no label mode) and hmsg_query_hier on it (declared below; the index of hmsg_graph_query belongs to the graph).
 *   hmsg_graph_to_json   ids, names and lists of every node + the edge list as one JSON text (buf NULL: *needed only). */
typedef struct hmsg_graph hmsg_graph_t;
typedef struct hmsg_index hmsg_index_t;
typedef struct hmsg_graph_params {
    int32_t num_views;          /* 24: KMeans clusters per room (graph.py:1136) */
    int32_t kmeans_n_init;      /* 5   (utils/graph_utils.py:329-333) */
    int32_t kmeans_max_iter;    /* 100 */
    uint32_t kmeans_seed;       /* 0   (random_state) */
    int32_t skip_frames;        /* pipeline.skip_frames: image id of processed frame i = i * skip_frames; <= 0: the handle's */
    int32_t image_width, image_height;   /* size of the views' images (check_object_in_view); 0: the handle's */
    double min_visible_ratio;   /* 0.5  (utils/graph_utils.py:95-157) */
    double max_view_depth;      /* 10.0 */
    int32_t host_threads;       /* KMeans fits / object writers; 0: one per core, at most 16 */
    int32_t merge_objects_graph;   /* pipeline.merge_objects_graph (graph.py:2053-2058; false in every shipped config): after the objects, every
                                    * room fuses its same-name objects whose clouds overlap (Room.merge_objects, hmsg_merge_room_objects with
                                    * the reference's 0.01 / 0.1) and re-numbers them; the graph's object list is then the rooms' lists */
    int32_t kmeans_device;      /* 0: the rooms' KMeans fits on host threads (hmsg_kmeans); != 0: the rooms of a storey in one hmsg_kmeans_batch
                                 * call on the device, from one worker thread -- the same bits either way */
} hmsg_graph_params;
typedef struct hmsg_graph_counts {
    int32_t floors, rooms, views, objects;
    int64_t edges, view_object_links;
    double begin_ms, finish_ms, kmeans_wait_ms;   /* wall time of the two halves; what finish waited for the KMeans threads */
} hmsg_graph_counts;
typedef struct hmsg_graph_object {
    char object_id[48];
    char name[80];
    int32_t room;               /* global room index (hmsg_graph_get_rooms order) */
    int32_t instance, label;    /* hmsg_node.instance / .label; -1 for a loaded graph */
    int32_t n_views, best_view; /* best_view: global view index, -1 none (loaded graphs: best_view_id resolved by hmsg_load) */
} hmsg_graph_object;
typedef struct hmsg_graph_room {
    char room_id[32];
    char name[80];
    int32_t floor;
    int64_t n_vertices, n_points;
    int32_t n_embeddings, n_sample_images, n_objects, n_views;
} hmsg_graph_room;
/* Lifetime: a BUILT graph (hmsg_build_graph / hmsg_graph_begin) keeps a plain reference to its scene handle -- the object clouds and
 * features stay in the handle's HBM -- so hmsg_graph_finish, hmsg_save, hmsg_graph_index and hmsg_graph_allgather_index need the
 * handle alive and not reset: destroy or reset the graph's scene only after hmsg_graph_destroy (a LOADED graph has no handle). */
void hmsg_graph_default_params(hmsg_graph_params* p);
int hmsg_build_graph(hmsg_t* h, const hmsg_graph_params* prm, int32_t n_frames, const double* poses, const double* poses_inv,
                     const float* view_feats, const char* const* img_paths, int32_t n_labels, const float* label_feats,
                     const char* const* label_names, hmsg_graph_t** out);
int hmsg_graph_begin(hmsg_t* h, const hmsg_graph_params* prm, int32_t n_frames, const double* poses, const double* poses_inv,
                     const float* view_feats, const char* const* img_paths, hmsg_graph_t** out);
int hmsg_graph_finish(hmsg_graph_t* g, int32_t n_labels, const float* label_feats, const char* const* label_names);
void hmsg_graph_destroy(hmsg_graph_t* g);
const char* hmsg_graph_last_error(const hmsg_graph_t* g);
int hmsg_graph_get_counts(const hmsg_graph_t* g, hmsg_graph_counts* counts);
int hmsg_graph_get_edges(const hmsg_graph_t* g, int64_t* edges /*[capacity][2], may be NULL*/, int64_t capacity, int64_t* n_edges);
int hmsg_graph_get_objects(const hmsg_graph_t* g, hmsg_graph_object* out, int64_t capacity);
int hmsg_graph_get_rooms(const hmsg_graph_t* g, hmsg_graph_room* out, int64_t capacity);
int hmsg_graph_get_room_vertices(const hmsg_graph_t* g, int32_t room, double* xz /*[n_vertices][2]: room.vertices*/, int64_t capacity);
int hmsg_graph_get_room_embeddings(const hmsg_graph_t* g, int32_t room, float* emb /*[n_embeddings][D]*/, int64_t capacity);
int hmsg_graph_to_json(const hmsg_graph_t* g, char* buf, int64_t capacity, int64_t* needed);
int hmsg_save(hmsg_graph_t* g, const char* dir);
int hmsg_load(const char* dir, int32_t device_id, hmsg_graph_t** out);
int hmsg_graph_index(hmsg_graph_t* g, const double* room_name_emb, hmsg_index_t** out);

/* ---- a graph against ground truth: the reference's evaluate_floors, evaluate_rooms and evaluate_objects
 * (memory/hmsg/eval/hm3dsem_evaluator.py:193-589) in one call.  Ground truth as plain arrays (the small ones in host memory; the point
 * arrays host or device):
 *   floors   floor_lower / floor_upper f64 [n_floors];
 *   rooms    bev clouds in CSR form (room_pts f64 [.][3], room_off i64 [n_rooms + 1]), room_min_h / room_max_h / room_mean_h f64;
 *   objects  clouds in CSR form, obb_center / obb_dims f64 [n_objects][3], obj_name_id i32 [n_objects]: the category as an id of
 *            the class table's names, -1 when the category is not in the vocabulary;
 *   classes  text_feats f32 [n_classes][feat_dim], class_name_id i32 [n_classes]: equal NAMES share an id. */
typedef struct hmsg_eval_gt {
    int32_t n_floors;
    const double *floor_lower, *floor_upper;
    int32_t n_rooms;
    const double* room_pts;
    const int64_t* room_off;
    const double *room_min_h, *room_max_h, *room_mean_h;
    int32_t n_objects;
    const double* obj_pts;
    const int64_t* obj_off;
    const double *obj_obb_center, *obj_obb_dims;
    const int32_t* obj_name_id;
    int32_t n_classes, feat_dim;
    const float* text_feats;
    const int32_t* class_name_id;
} hmsg_eval_gt;
enum { HMSG_EVAL_IOU = 0, HMSG_EVAL_OVERLAP = 1 };
typedef struct hmsg_eval_params {
    int32_t eval_metric;          /* HMSG_EVAL_*: which matrix the objects are assigned on (:460-465); the sweep is on the overlaps either way */
    double room_radius;           /* 0.05 */
    double object_radius;         /* 0.02 */
    double voxel;                 /* 0.05: the rooms' bev down-sampling */
    int32_t n_top_k;
    const int32_t* top_k;         /* params.eval.hm3dsem.top_k_object_semantic_eval */
} hmsg_eval_params;
void hmsg_eval_default_params(hmsg_eval_params* p);      /* overlap, 0.05, 0.02, 0.05, no top_k list */
/* every key of the reference's three dictionaries */
typedef struct hmsg_eval_metrics {
    hmsg_eval_counts floors;                              /* metrics["floors"]: tp tn fp fn acc prec recall */
    double room_acc50, room_ap, room_prec50, room_recall50;   /* metrics["rooms"]: "acc@IoU=0.5", "ap", "prec@IoU=0.5", "recall@IoU=0.5" */
    int32_t room_gt, room_pred;
    double room_hydra_prec, room_hydra_recall;
    double obj_ap;                                        /* metrics["objects"]["instances"]: ap, gt, pred */
    int32_t obj_gt, obj_pred;
    hmsg_eval_counts obj_iou50;                           /* ["instances_iou50"]: acc prec recall tp fp fn (gt, pred as above) */
    double obj_top_k_auc;                                 /* ["ins_semantics"]["top_k_auc"]; "tp_top_k_acc" goes to the top_k_acc array */
    int32_t obj_assigned;                                 /* len(col_ind) */
} hmsg_eval_metrics;
/* Works on a built graph (room clouds from the storeys' slabs of the map, objects from the scene's instances and pooled features --
 * what hmsg_save writes) and on a loaded one (the clouds and float64 embeddings hmsg_load read; the device work runs on a small
 * scene handle of the call's own).  Composes hmsg_eval_floors, hmsg_eval_rooms, hmsg_eval_object_matrices, hmsg_lsap,
 * hmsg_eval_semantic_ranks and the metrics of csrc/hmsg_eval_metrics_host.h.  top_k_acc f64 [n_top_k] (may be NULL when n_top_k is
 * 0); prm NULL: the defaults.  HMSG_ERR_INVALID (text in hmsg_graph_last_error): unequal floor counts, no rooms or no objects on
 * a side, feat_dim that is not the graph's, an object without an embedding. */
int hmsg_graph_evaluate(hmsg_graph_t* g, const hmsg_eval_gt* gt, const hmsg_eval_params* prm, hmsg_eval_metrics* out, double* top_k_acc);
int hmsg_graph_query(hmsg_graph_t* g, const double* room_name_emb, int32_t Q, int32_t C, const float* T_obj, const int32_t* qid,
                     const float* T_room, const int32_t* floor_id, const int32_t* room_mode, int32_t k, int32_t use_negatives,
                     int32_t max_rooms, int32_t* out_sel, int32_t* out_nsel, int32_t* out_idx, int32_t* out_room, double* out_score);

/* ---- room names: the step between hmsg_load and a label-mode query in the reference's query applications
 * (load_hmsg_graph; generate_room_names(generate_method="obj_embedding", default_room_types=[...]); query_hierarchy_protected_icra).
 *   hmsg_graph_name_rooms  Graph.generate_room_names (graph.py:2146-2187) for n_types room types: type_feats f32 [n_types][D] = the
 *        text features of the type names (get_text_feats_multiple_templates(default_room_types)), type_names [n_types].
 *          HMSG_ROOM_NAMES_OBJ_EMBEDDING   Room.infer_room_type_from_objects(infer_method="obj_embedding") (room.py:237-308):
 *              feats_denoise_dbscan (utils/graph_utils.py:682-728: eps 0.02, min_samples 2, cosine) of the room's object embeddings
 *              (float64 on a loaded graph, the float32 pooled features on a built one), then the first arg-max of
 *              represent . type_feats^T.  A room without objects: HMSG_ERR_INVALID naming the room (sklearn raises on an empty
 *              array) and no room is renamed.
 *          HMSG_ROOM_NAMES_VIEW_EMBEDDING  Room.infer_room_type_from_view_embedding (room.py:131-172): per view embedding the
 *              arg-max over the types, the majority vote (ties: the smallest type id); a room without views keeps its name.
 *        type_of_room [rooms] (optional) receives the chosen type per room in hmsg_graph_get_rooms order, -1 where the name was
 *        left unchanged.  The new names show in hmsg_graph_get_rooms, hmsg_graph_to_json and hmsg_save; the graph's query index is
 *        dropped, so that the next hmsg_graph_query makes it again with the room_name_emb it is given.
 *        Label mode from C: the text feature of a room's name is the type table's row of its type, so
 *            room_name_emb[r][d] = (double)type_feats[type_of_room[r]][d]
 *        for every room with type_of_room[r] >= 0 (a room whose name was left unchanged needs the feature of its own name).
 *   hmsg_graph_set_room_names  Graph.set_room_names (graph.py:2129-2144, the applications' "human_assign" mode): n must be the
 *        number of rooms (the reference asserts it); the room centre the reference also stores is not part of the graph object.
 *   hmsg_denoise_feats_batch  feats_denoise_dbscan (utils/graph_utils.py:682-728, sklearn 1.7.2 semantics) of n_sets sets at once:
 *        set k = rows set_off[k] .. set_off[k + 1] of feats [.][dim] (f32, or f64 when feats_is_f64), set_off host int64
 *        [n_sets + 1], no set empty (HMSG_ERR_INVALID: sklearn raises).  Rows are L2-normalised (zero rows stay zero),
 *        d = 1 - x.y clipped to [0, 2] with a zero diagonal, neighbours iff d <= eps, core rows have >= min_samples neighbours
 *        (themselves included).  out [n_sets][dim] in the input dtype: the mean of the largest cluster's rows (ties: the
 *        cluster that appears first in row order, Counter.most_common), added in row order and divided by their number as
 *        np.mean(axis=0) does; with no cluster the mean of all rows.  n_in_cluster (host int32 [n_sets], optional): rows of
 *        that cluster, 0 = no cluster.  feats / out: host or device pointers. */
#define HMSG_ROOM_NAMES_OBJ_EMBEDDING 1
#define HMSG_ROOM_NAMES_VIEW_EMBEDDING 2
int hmsg_graph_name_rooms(hmsg_graph_t* g, int32_t method, int32_t n_types, const float* type_feats, const char* const* type_names,
                          int32_t* type_of_room);
int hmsg_graph_set_room_names(hmsg_graph_t* g, int32_t n, const char* const* names);
int hmsg_denoise_feats_batch(int32_t device_id, int32_t n_sets, const int64_t* set_off, const void* feats, int32_t feats_is_f64, int32_t dim,
                             double eps, int32_t min_samples, void* out, int32_t* n_in_cluster);

/* ---- A12: retrieval over a node table (graph.py:3056-3162 query_hmsg_object and the GEMV of
 * query_hmsg_room / query_floor).  A table is N node embeddings (f64, as after load_hmsg_graph:
 * object.py:88-89, or f32 right after build) with a parent (room) id per node. */
int hmsg_index_create(int32_t device_id, int32_t dim, int64_t n, const void* emb, int32_t emb_is_f64,
                      const int32_t* room_of_node, hmsg_index_t** out);
/* the node table of a built scene as a resident index (embeddings gathered on the device, parent = node.room) */
int hmsg_index_from_nodes(hmsg_t* h, hmsg_index_t** out);
void hmsg_index_destroy(hmsg_index_t* ix);
const char* hmsg_index_last_error(const hmsg_index_t* ix);
/* live HIP-event timing of the similarity GEMM on the index's stream (measurement aid for bench.py) */
int hmsg_index_set_profiling(hmsg_index_t* ix, int32_t on);
int hmsg_index_profile(hmsg_index_t* ix, int64_t* launches, double* total_ms, double* total_flop);
/* Q queries; query q has C text rows T[q][C][D] f32 (row `qid[q]` is the query itself, the others
 * the negative prompts), searches the nodes whose room id is listed in rooms[room_off[q] ..
 * room_off[q+1]) IN THAT ORDER (candidate order = room order then node order, graph.py:3099-3110),
 * returns up to k node indices (-1 padded), their room ids and float64 scores sim[qid][node]. */
int hmsg_query_objects(hmsg_index_t* ix, int32_t Q, int32_t C, const float* T, const int32_t* qid,
                       const int32_t* room_off, const int32_t* rooms, int32_t k, int32_t use_negatives,
                       int32_t* out_idx, int32_t* out_room, double* out_score);
/* ---- the coarse-to-fine query behind the drivers query_hierarchy_protected{,_icra} (graph.py:3483-3716): floor ->
 * room(s) -> objects, batched, every stage on the device.
 *   hmsg_index_set_hierarchy  makes the levels above the nodes resident: n_rooms rooms (rooms without objects count), the rooms of every floor in floors[f].rooms
 *        order (CSR floor_room_off [n_floors + 1] / floor_rooms; room ids as in room_of_node, where self.rooms order =
 *        ascending id), per room the CLIP embedding of its NAME (room_name_emb f64 [R][D]; NULL: no label mode), its
 *        view embeddings room.embeddings (CSR view_off i64 [R + 1] / view_emb f64 [NV][D]) and room_key[r] =
 *        int(room_id.split("_")[-1]), the number the view mode reports (graph.py:3254-3262).
 *   hmsg_query_hier  per query: floor_id (-1 = all rooms; resolve query_floor :2216-2257 on the host or with
 *        hmsg_similarity), the room text row T_room[q][D] and room_mode[q]:
 *          0  no room stage: every room of the floor's list;
 *          1  query_hmsg_room(..., "label") (:3204-3232): rooms whose name similarity is within 1e-3 of the best;
 *          2 / 3  the view-embedding branch (:3247-3272): the 5 (valid room text) / 10 best rooms by their best view;
 *        then query_hmsg_object (:3056-3162) over those rooms IN THAT ORDER with the C text rows T_obj[q] (row qid[q] the
 *        query, the others negative prompts).  out_sel [Q][max_rooms] / out_nsel [Q]: the numbers query_hmsg_room
 *        returns (positions in the floor's room list; in view mode the room keys, which the reference then uses AS
 *        positions); out_idx / out_room / out_score [Q][k] as hmsg_query_objects (room = global room id).
 *        HMSG_ERR_INVALID where the reference raises (a room without view embeddings in view mode; a key that is no
 *        position of the list). */
int hmsg_index_set_hierarchy(hmsg_index_t* ix, int32_t n_rooms, int32_t n_floors, const int32_t* floor_room_off, const int32_t* floor_rooms,
                             const double* room_name_emb, const int64_t* view_off, const double* view_emb, const int32_t* room_key);
int hmsg_query_hier(hmsg_index_t* ix, int32_t Q, int32_t C, const float* T_obj, const int32_t* qid, const float* T_room,
                    const int32_t* floor_id, const int32_t* room_mode, int32_t k, int32_t use_negatives, int32_t max_rooms,
                    int32_t* out_sel, int32_t* out_nsel, int32_t* out_idx, int32_t* out_room, double* out_score);
/* plain similarity S[Q][N] = T[Q][D] . E[N][D]^T in float64 (query_floor / query_hmsg_room GEMV) */
int hmsg_similarity(hmsg_index_t* ix, int32_t Q, const float* T, double* S);

/* ---- multi-GPU exchange steps: RCCL collectives on device buffers, issued by the host that drives the handle.
 * The reference has no multi-GPU path: its benchmark driver loops scenes one after the other
 * (application/.../offline_mapping_create_hmsg_hm3d_benchmark.py:70-110) -- one process per GPU builds its own scene with no
 * collective, and these calls are the only exchange steps.  librccl is loaded on first use (a one-GPU process never needs
 * it).  One communicator per process / GPU:
 *   hmsg_comm_unique_id   rank 0 makes the 128-byte id (ncclGetUniqueId); the host passes it to the other ranks by its own
 *                         means (MPI, a TCP store, torch.distributed's store ...);
 *   hmsg_comm_create      ncclCommInitRank on device_id.  id == NULL with world == 1: no communicator, every collective is
 *                         the identity (single-GPU runs take the same code path). */
#define HMSG_COMM_ID_BYTES 128
typedef struct hmsg_comm hmsg_comm_t;
int hmsg_comm_unique_id(uint8_t* out_id /* [HMSG_COMM_ID_BYTES] */);
int hmsg_comm_create(const uint8_t* id, int32_t rank, int32_t world, int32_t device_id, hmsg_comm_t** out);
void hmsg_comm_destroy(hmsg_comm_t* c);
const char* hmsg_comm_last_error(const hmsg_comm_t* c);
/* Cross-scene retrieval (configs[3]): all-gather of the ranks' node tables -- embeddings of the object nodes gathered on
 * the device (f32 [n][D]) and the parent room of every node -- into ONE resident index on every rank (counts first, then
 * the payload padded to the largest table, HBM to HBM).  Global node index = node_off[rank] + local index, global room id =
 * room_off[rank] + local room id (n_rooms_local = rooms of this rank's graph, rooms without objects included); the index
 * answers like hmsg_index_create over the concatenated tables.  node_off / room_off: [world + 1], optional. */
int hmsg_allgather_nodes(hmsg_t* h, hmsg_comm_t* c, int32_t n_rooms_local, hmsg_index_t** out_index, int64_t* node_off, int64_t* room_off);
/* The same with the levels above the nodes (configs[3] through the graph object): every rank's graph -> ONE resident index on every
 * rank -- node tables as above, plus floors -> rooms, the rooms' keys and view embeddings and (on every rank or on none) the embeddings of
 * the rooms' names, all with global ids: room = room_off[rank] + local, floor = floor_off[rank] + local ([world + 1] each, optional).
 * hmsg_query_hier on the result addresses a storey by its global floor id.  (The benchmark driver used to gather these tables as
 * pickled Python objects inside its timed step.) */
int hmsg_graph_allgather_index(hmsg_graph_t* g, hmsg_comm_t* c, const double* room_name_emb, hmsg_index_t** out, int64_t* node_off,
                               int64_t* room_off, int64_t* floor_off);
/* Point to point: `bytes` of a DEVICE buffer to / from rank dst / src (ncclSend / ncclRecv on the handle's stream; returns when the
 * transfer has completed).  The cross-rank joins of the sharded merge tree are made of these; a host that schedules them itself can
 * use the pair directly. */
int hmsg_comm_send(hmsg_t* h, hmsg_comm_t* c, const void* dev_buf, int64_t bytes, int32_t dst);
int hmsg_comm_recv(hmsg_t* h, hmsg_comm_t* c, void* dev_buf, int64_t bytes, int32_t src);
/* hierarchical_merge (graph_utils.py:989-1012) of ONE episode whose frame windows are spread over the ranks (configs[4]), one call
 * per rank after hmsg_fuse_frames (+ hmsg_allreduce_feature_sums): the levels inside the rank's window (hmsg_merge_tree_local), the
 * ranks' agreement on the level they meet at (an all-gather of 16 bytes), then level by level the owner of list 2k + 1 sends its
 * clouds -- count, sizes, points, HBM to HBM -- to the owner of list 2k, which merges [mine ++ theirs] (hmsg_merge_tree_join; the
 * last join runs the final pass).  Any number of ranks whose windows are subtrees of the merge tree (hmsg_set_frame_window).
 * *holds_result = 1 on the rank that ends with the episode's instances (the rank of frame 0), bit-identical to a one-process
 * hmsg_merge_instances; hmsg_pool_instances follows there.  Until round 5 this schedule lived in Python over torch.distributed. */
int hmsg_merge_tree_sharded(hmsg_t* h, hmsg_comm_t* c, int32_t total_frames, int32_t* holds_result);
/* One episode fused in disjoint frame windows (configs[4]): the per-voxel feature sums and frame counters of all ranks are
 * all-reduced in place (graph.py:410-415: `sum[idx] += F; cnt[idx] += 1` over the frames commute across windows; counters
 * exact, float32 sums up to summation order) and the voxel features refreshed.  After hmsg_fuse_frames, before pooling. */
int hmsg_allreduce_feature_sums(hmsg_t* h, hmsg_comm_t* c);

/* ---- the sharded query (scene per GPU): hmsg_query_hier over several scene graphs whose tables stay where they are.
 * Contract: for the same queries the answer is, bit for bit, what hmsg_query_hier returns on ONE index over the concatenated tables
 * (the index hmsg_graph_allgather_index makes for built graphs) -- out_sel, out_nsel, out_idx, out_room and the float64 out_score, every
 * room mode, floor -1 or any global floor id, use_negatives 0 / 1, any k, and HMSG_ERR_INVALID where hmsg_query_hier raises (a room
 * without view embeddings in view mode; a view key that is no position of the list; the outputs are written first, as there).
 * Global ids, in shard order 0 .. n-1 (= rank order): node = node_off[s] + local node, room = room_off[s] + local room, floor =
 * floor_off[s] + local floor (offsets [n + 1], optional).  Shards may be built graphs (hmsg_graph_finish), loaded graphs (hmsg_load) or
 * a mix; a graph without objects takes part with its rooms.  Every table is float64 in HBM on its own shard: each graph keeps its own
 * resident index for this path (made on the first call, without room names -- they come with every call; the index hmsg_graph_query
 * makes and caches is not touched) and its scratch, both freed with the graph.
 * room_name_emb: the shard's rooms [R_local][D] f64 (host or device) or NULL; when any query is in label mode it must be given on every
 * shard -- a shard without it makes every shard return HMSG_ERR_INVALID.
 * max_rooms: the capacity of out_sel [Q][max_rooms]; hmsg_query_hier's callers pass max(rooms of the concatenated table, 10), and
 * the same here gives the same sel (a smaller value cuts sel, the same way on both).  Q = 0 reads no query array: the call is the
 * header exchange alone and fills the offsets, e.g. room_off[n] to size max_rooms.
 *   hmsg_graph_query_sharded  one call per rank, every rank with the same queries; every rank receives the whole answer.  The first
 *        exchange carries every rank's own preconditions (arguments, graph finished, label mode with room_name_emb, D) and its query
 *        arguments (Q, C, k, max_rooms, use_negatives, a hash of the floor ids and room modes): a rank that fails them, or differs, makes
 *        every rank return HMSG_ERR_INVALID -- nobody is left waiting -- and every rank-local phase after it ends in an agreement (a 4-byte
 *        all-reduce).  With c from hmsg_comm_create(NULL, 0, 1, ...) (one rank, no communicator) it equals hmsg_graph_query.
 *        What ONE rank receives per call (its own slot included; summed over W ranks about W times this), R = the largest room count of
 *        a rank, F / FR its floor count / floor-list length:
 *          the header all-gather   W x 128 bytes;
 *          the room all-gather     W x [Q*R*8 per room row kind in use (label names; views: the best view per room) + 4*(F + 1 + FR + 2R)],
 *                                  each section rounded up to 16 bytes;
 *          the candidate all-gather  W x [Q*2k*24 + Q*4] (k plain + k negative-filtered records, and a count, per query),
 *        plus the 4-byte agreements.  No table is gathered: a changed, reloaded or added scene changes nothing on the other ranks.
 *   hmsg_graphs_query  the same answer for n graphs held by this process on ONE device (a multi-building service): no communicator,
 *        each shard writes its slots of the exchange in place on one stream. */
int hmsg_graph_query_sharded(hmsg_graph_t* g, hmsg_comm_t* c, const double* room_name_emb, int32_t Q, int32_t C, const float* T_obj,
                             const int32_t* qid, const float* T_room, const int32_t* floor_id, const int32_t* room_mode, int32_t k,
                             int32_t use_negatives, int32_t max_rooms, int32_t* out_sel, int32_t* out_nsel, int32_t* out_idx, int32_t* out_room,
                             double* out_score, int64_t* node_off, int64_t* room_off, int64_t* floor_off);
int hmsg_graphs_query(int32_t n, hmsg_graph_t* const* graphs, const double* const* room_name_embs, int32_t Q, int32_t C, const float* T_obj,
                      const int32_t* qid, const float* T_room, const int32_t* floor_id, const int32_t* room_mode, int32_t k, int32_t use_negatives,
                      int32_t max_rooms, int32_t* out_sel, int32_t* out_nsel, int32_t* out_idx, int32_t* out_room, double* out_score,
                      int64_t* node_off, int64_t* room_off, int64_t* floor_off);

/* ---- the view level of the slow path: what Graph.query_room_obj_slow_reasoning (graph.py:2578-3054) computes between its VLM calls,
 * on the graph object (holoagent_amd/csrc/hmsg_query_views.hip).  The caller keeps detect_object_in_image, vlm_choose,
 * detect_and_select_best_gpt and the drawing; INTEGRATION.md maps the steps.
 *   hmsg_graph_get_views   per view, in self.views order: its index, img_id (-1: none), room (hmsg_graph_get_rooms order, -1: none) and
 *        the length of its object list.
 *   hmsg_graph_get_view_objects   that list: find_object_by_object_id (graph.py:2572-2576: the first object that carries the id) of
 *        every entry of view.object_ids, in that order (:2968-2973), as indices of hmsg_graph_get_objects; an id that no object carries
 *        -- the reference asserts there -- is left out.
 *   hmsg_graph_find_view   find_view_by_imgpath (graph.py:2566-2570): the first view in view order whose img_path equals img_path, or,
 *        with img_path NULL, whose img_id equals img_id; *view = -1 when there is none.
 *   hmsg_graph_object_best_views   graph.py:2759-2765 + :2828-2831: view[i] = the view that carries obj[i]'s best_view_id (-1: none --
 *        the reference's best_view = None), img_id[i] (optional) its image.  hmsg_graph_object::best_view holds the same index on built
 *        and, since hmsg_load resolves best_view_id / view_ids, on loaded graphs; an id that names no view stays -1.
 *   hmsg_graph_goal_views   graph.py:2864-2897 for Q object texts T f32 [Q][D] (host or device) at once: the text against the CLIP
 *        embedding of every sampled image (room.sample_images / room.clip_embeddings) of every room of the query's list -- all rooms
 *        for floor_id[q] = -1, floors[f].rooms in that order otherwise.  The table is float64 in HBM, made on the first call and freed
 *        with the graph; scores come from the float64 MFMA GEMM of hmsg_similarity.  out_img i64 / out_room i32 (global room index) /
 *        out_score f64 [Q][k], out_n [Q] (host or device): the k best rows (k = 24 in the reference, any k >= 1), -1 / -1 / 0.0 past
 *        out_n[q] = min(k, rows of the list); no sampled image at all gives out_n = 0.
 *        ORDER: descending score; exact ties (bit-equal scores) by ascending candidate position = place of the room in the list, then
 *        place of the image in the room.  Row 0 is therefore np.argmax(sims) (first maximum), and the rest is
 *        np.argsort(sims)[-k:][::-1] wherever scores differ; numpy's order of bit-equal keys is undefined, so there only the set of
 *        tied rows compares (the rule of hmsg_query_objects).
 *        A room of the list whose sample_images and clip_embeddings differ in length: HMSG_ERR_INVALID naming the room (the
 *        reference asserts, :2870).
 *   hmsg_graph_rematch_in_views   graph.py:2962-2986 for Q (text row, view index) pairs: the text against the embeddings of the
 *        view's object list in that order, the FIRST maximum (np.argmax).  out_obj [Q] (index of hmsg_graph_get_objects, -1 for a view
 *        without objects: the reference skips it, :2974), out_score f64 [Q] -- bit for bit hmsg_similarity's entry for that (text row,
 *        object) on the graph's index, 0.0 with -1.  With pose_inv f64 [Q][16] (world -> camera of the view's image: np.linalg.inv(pose)
 *        as the reference makes it), wh i32 [Q][2] (image width, height) and K f64 [9]: out_avg_distance f64 [Q] =
 *        visualize_pcd_on_image's avg_distance of the chosen object (utils/graph_utils.py:49-70: the mean camera z of its points with
 *        z > 0; NaN where the reference returns None -- no such point, an empty cloud, out_obj -1).  pose_inv NULL: no distances.
 *        The cloud is the object's as the graph holds it: the instance cloud in HBM on a built graph (the concatenated parts after
 *        merge_objects_graph), the saved cloud on a loaded one (uploaded once, cached, freed with the graph).
 *   hmsg_graph_object_view_depths   graph.py:3011-3022: check_object_in_view(w, h, K, pose_inv, points, return_depth=True)
 *        (utils/graph_utils.py:95-157) of n (object, camera) pairs with the graph's min_visible_ratio / max_view_depth: visible u8 [n],
 *        mean_depth f64 [n] exactly as hmsg_object_views defines them (inf where the reference returns inf).
 * Host arrays: floor_id (hmsg_graph_goal_views), view (hmsg_graph_rematch_in_views), obj, pose_inv, wh and K are read on the host and
 * must be host memory; only T and the outputs named "host or device" may be device pointers (the table-level hmsg_rematch_in_views also
 * takes a device `view`).  Lifetime: on a BUILT graph hmsg_graph_rematch_in_views with pose_inv and hmsg_graph_object_view_depths read the
 * object clouds in the scene handle's HBM, so the handle must be alive and not reset (as for hmsg_save); a LOADED graph needs none.
 * Errors: an unfinished or failed graph (every call of this group, the listing calls included), a view / object / floor index out of
 * range: HMSG_ERR_INVALID, text in hmsg_graph_last_error.
 * Table level, for hosts that keep their own tables (and for tests of the kernels' edges):
 *   hmsg_index_set_views   CSR view -> nodes of an index (view_obj_off i64 [n_views + 1] from 0, view_objs i32, in object_ids order);
 *   hmsg_rematch_in_views  the re-match on it: T host or device, view host or device, outputs host or device;
 *   hmsg_points_view_depths   pair p = points pts_off[p] .. pts_off[p + 1] of pts f64 [.][3] (host or device) through pose_inv [p][16],
 *        wh [p][2], K [9] (host): avg_z_front, visible, mean_depth [n_pairs] (host, each optional).  Sums are float64 in a fixed order
 *        (two stages, no floating-point atomics): the same input gives the same bits on every run. */
typedef struct hmsg_graph_view {
    int32_t view;               /* global view index (self.views order) */
    int32_t room;               /* global room index, -1 none */
    int64_t img_id;             /* View.img_id, -1 none */
    int32_t n_objects;          /* length of hmsg_graph_get_view_objects' list */
    int32_t reserved_;
} hmsg_graph_view;
int hmsg_graph_get_views(hmsg_graph_t* g, hmsg_graph_view* out, int64_t capacity);
int hmsg_graph_get_view_objects(hmsg_graph_t* g, int32_t view, int32_t* obj, int64_t capacity);
int hmsg_graph_find_view(hmsg_graph_t* g, const char* img_path, int64_t img_id, int32_t* view);
int hmsg_graph_object_best_views(hmsg_graph_t* g, int32_t n, const int32_t* obj, int32_t* view, int64_t* img_id);
int hmsg_graph_goal_views(hmsg_graph_t* g, int32_t Q, const float* T, const int32_t* floor_id, int32_t k, int64_t* out_img, int32_t* out_room,
                          double* out_score, int32_t* out_n);
int hmsg_graph_rematch_in_views(hmsg_graph_t* g, int32_t Q, const float* T, const int32_t* view, const double* pose_inv, const int32_t* wh,
                                const double* K, int32_t* out_obj, double* out_score, double* out_avg_distance);
int hmsg_graph_object_view_depths(hmsg_graph_t* g, int32_t n, const int32_t* obj, const double* view_pose_inv, const int32_t* wh, const double* K,
                                  uint8_t* visible, double* mean_depth);
int hmsg_index_set_views(hmsg_index_t* ix, int64_t n_views, const int64_t* view_obj_off, const int32_t* view_objs);
int hmsg_rematch_in_views(hmsg_index_t* ix, int32_t Q, const float* T, const int32_t* view, int32_t* out_node, double* out_score);
int hmsg_points_view_depths(int32_t device_id, int64_t n_pairs, const int64_t* pts_off, const double* pts, const double* pose_inv, const int32_t* wh,
                            const double* K, double min_visible_ratio, double max_depth, double* avg_z_front, uint8_t* visible, double* mean_depth);

/* ---- N6: the image half of a floor's navigation graph (graph/navigation_graph.py NavigationGraph; csrc/hmsg_navmap.hip,
 * csrc/hmsg_nav_host.h): a storey's cloud -> the grid maps of get_main_free_map, the boundary cells get_voronoi_graph hands to
 * scipy.spatial.Voronoi, and the top-down image of get_top_down_rgb_map.  Images are [grid[1] rows (z)][grid[0] columns (x)],
 * row-major.  Every output is exact (integer work; the obstacle map is a whole number of sixteenths).  The rules:
 *   1. cell of a coordinate: floor((v - pcd_min) / cell_size) in float64 (subtract, then divide); pcd_min / pcd_max are the
 *      bounds of ALL points of the storey, grid = int32(ceil((pcd_max - pcd_min) / cell_size + 1)) for x and z (:57-65);
 *   2. obstacle points: zero_level + obstacle_lo < y < zero_level + obstacle_hi (:163-167); region points and the points of the
 *      top-down image: y < zero_level + region_max (:193-195, :462); the sums are formed in float64 first;
 *   3. create_occupancy_grid (:230-240): cv2.dilate by a dilation x dilation box (the window clipped at the border), then
 *      cv2.GaussianBlur 3 x 3 = (1, 2, 1) x (1, 2, 1) / 16 in float32, the border reflected without repeating the edge.
 *      obstacle_map is that float32 image of the obstacle cells (NavigationGraph.map), region_map = (that of the region cells) > 0;
 *   4. poses_map (get_poses_region :348-377): sklearn's DBSCAN(eps = pose_eps, min_samples = pose_min_samples) on the poses'
 *      heights (pose[1][3]; neighbours at distance <= eps, clusters numbered by their first core sample, noise -1), the most
 *      frequent label (of equally frequent ones the smallest: noise wins a tie), the mean height of that label (numpy's pairwise
 *      sum), keep |h - mean| < pose_eps, then h < min + pose_eps; cell = int32((xz - pcd_min) / cell_size) truncated toward zero;
 *      a filled cv2.circle of radius int(pose_radius / cell_size) round each, clipped to the image.  The circle is OpenCV's
 *      midpoint walk restated without an OpenCV to compare with;
 *   5. free_map = (region_map or poses_map) and obstacle_map == 0 (:414-421);
 *   6. get_largest_region (:316-322): 8-connected components of free_map, labels in raster order of each component's first
 *      cell, label 0 the background.  region_rule 0 (the reference): the label SECOND in descending order of area, the
 *      background counted -- which is the background itself when the free region is the larger of the two; region_rule 1: the
 *      largest component.  Of equal areas the larger label comes first (np.argsort leaves it open).  main_free_map = (labels ==
 *      main_label); main_area its cells; n_regions = labels, the background included;
 *   7. boundary_rc: the cells of main_free_map with a 4-neighbour outside it (outside the image counts), as (row, col) in
 *      row-major order = np.argwhere(main - binary_erosion(main)) (:511-521): Qhull numbers vertices and ridges by input order;
 *   8. top_down_bgr (:458-481; only with colours): per cell the point with the greatest height cell int32((y - pcd_min[1]) /
 *      cell_size) wins, of equal ones the lowest index; its colour is uint8(c * 255) truncated (c in [0, 1]); empty cells are 0;
 *      scipy.ndimage.median_filter(size = 3) over the (rows, cols, 3) array, the channel axis included, mode reflect; stored B, G, R.
 * Any output pointer of hmsg_nav_maps may be NULL (not wanted) and may be host or device memory, as may xyz, rgb and poses.
 * Errors (HMSG_ERR_INVALID unless said): a null prm / xyz / out; no points; a coordinate of any point of the cloud that is not
 * finite (NaN or infinite; counted on the device, outside a graph's slab too); no pose (n_poses == 0), a pose height pose[1][3] that
 * is not finite (a pose's x / z may be anything: its cell is clamped far outside the grid), or none left by rule 4 (the reference
 * raises); no free cell (fewer than two labels); boundary_capacity < n_boundary (the maps
 * are written, the list is not, n_boundary says what is needed); HMSG_ERR_UNSUPPORTED for a blur other than 3 or 0 and for a
 * grid of 2^28 cells or more.  pcd_min, pcd_max and grid are set as soon as the cloud has been read. */
typedef struct hmsg_nav_params {
    double  cell_size;          /* 0.03 m */
    double  obstacle_lo;        /* 1.4 */
    double  obstacle_hi;        /* 2.5 */
    double  region_max;         /* 1.5 */
    double  pose_radius;        /* 0.5 m */
    double  pose_eps;           /* 0.1: DBSCAN's eps and both height filters */
    int32_t dilation;           /* 5; 0 = none */
    int32_t blur;               /* 3; 0 = none */
    int32_t pose_min_samples;   /* 5 */
    int32_t region_rule;        /* 0 = the reference's second-largest label, 1 = the largest component */
} hmsg_nav_params;
typedef struct hmsg_nav_maps {
    float*   obstacle_map;      /* f32 [H][W] */
    uint8_t* region_map;        /* u8 [H][W], 0/1, like the next three */
    uint8_t* poses_map;
    uint8_t* free_map;
    uint8_t* main_free_map;
    uint8_t* top_down_bgr;      /* u8 [H][W][3] */
    int32_t* boundary_rc;       /* i32 [boundary_capacity][2] */
    int64_t  boundary_capacity;
    /* out */
    int64_t  n_boundary;
    int64_t  main_area;
    int32_t  n_regions;
    int32_t  main_label;
    int32_t  grid[2];           /* columns (x), rows (z) */
    double   pcd_min[3], pcd_max[3];
} hmsg_nav_maps;
void hmsg_nav_default_params(hmsg_nav_params* p);
/* the size call: bounds and grid of xyz f64 [n][3] (pcd_min, pcd_max: f64 [3], optional; grid: i32 [2]; host memory) */
int hmsg_nav_grid(int32_t device_id, double cell_size, int64_t n, const double* xyz, double* pcd_min, double* pcd_max, int32_t* grid);
/* the work call: rgb f64 [n][3] or NULL (no top-down image), poses f64 [n_poses][16] (row-major camera-to-world 4 x 4) */
int hmsg_nav_floor_maps(int32_t device_id, const hmsg_nav_params* prm, int64_t n, const double* xyz, const double* rgb, double zero_level,
                        int32_t n_poses, const double* poses, hmsg_nav_maps* out);
/* The same stage on storey `floor` of a built graph: the map points with y_lo <= y <= y_hi in map order with their colours (the
 * slab hmsg_save writes as floors/<f>.ply), selected on the device, zero_level the floor's own.  A graph read by hmsg_load has no
 * cloud in HBM and is refused (HMSG_ERR_INVALID; its caller gives hmsg_read_ply's points to hmsg_nav_floor_maps). */
int hmsg_graph_nav_grid(hmsg_graph_t* g, int32_t floor, double cell_size, double* pcd_min, double* pcd_max, int32_t* grid);
int hmsg_graph_nav_floor_maps(hmsg_graph_t* g, int32_t floor, const hmsg_nav_params* prm, int32_t n_poses, const double* poses,
                              hmsg_nav_maps* out);
/* ... and on a slab y_lo <= y <= y_hi of a scene's finalised map (what hmsg_segment_floors returns for a storey), for callers that
 * hold the scene and no graph handle; zero_level is theirs to give (hmsg_floor.zero_level). */
int hmsg_map_nav_grid(hmsg_t* h, double y_lo, double y_hi, double cell_size, double* pcd_min, double* pcd_max, int32_t* grid);
int hmsg_map_nav_floor_maps(hmsg_t* h, double y_lo, double y_hi, double zero_level, const hmsg_nav_params* prm, int32_t n_poses,
                            const double* poses, hmsg_nav_maps* out);

/* ---- N7: routes on a floor's free map (csrc/hmsg_navroute.hip): exact distance fields of the grid graph, the clearance of a
 * mask, the nearest candidate cell of a target, the cells of the way.  The reference has no such stage (navigation_graph.py:23,36
 * imports skfmm and defines compute_sdf, which nothing calls; goal_pose_publisher.py:260-271 publishes an object's centre as it
 * is), so the rules are this library's.  Images are [rows (z)][cols (x)], row-major, as in N6; cells are (row, col) int32 pairs
 * like boundary_rc; a cell is passable / in the mask where its byte is not 0.  Every array may be host or device memory.  All
 * of it is integer work: every output has one right answer.  The rules:
 *  R1. Moves: the eight neighbours in this fixed order: N (-1, 0), S (+1, 0), W (0, -1), E (0, +1), NW (-1, -1), NE (-1, +1),
 *      SW (+1, -1), SE (+1, +1).  A straight move costs w_straight, a diagonal one w_diag (5 and 7: metres = value * cell_size
 *      / 5).  A move is legal when both cells are passable; a diagonal move also needs both cells it squeezes between to be
 *      passable (no corner cutting: [[1, 0], [0, 1]] is two islands).
 *  R2. Field: field[c] = the least cost of a legal walk from any source cell of the set to c, int32.  HMSG_NAV_UNREACHED marks
 *      every cell no walk reaches and every cell that is not passable.  A source on a cell that is not passable is no source;
 *      an empty set gives an all-unreached field; duplicate sources are fine.  n_reached[s] counts the finite cells.
 *  R3. Clearance: 0 outside the mask; inside, the least cost to the nearest cell not in the mask, every move allowed (no corner
 *      rule, the walk may cross anything), cells outside the image counting as not in the mask: a full mask gives
 *      w_straight * (1 + min(r, rows - 1 - r, c, cols - 1 - c)).
 *  R4. Snap: for a target cell, the candidate minimising d2 = dr * dr + dc * dc (int64, the target's indices clamped to
 *      [-2^20, 2^20] first); of equal d2 the smaller row-major index.  Candidates: the passable cells; with a field, the passable
 *      cells whose field value is finite.  No candidate: cell (-1, -1) and d2 = -1.
 *  R5. Path: from the field's source to a goal cell, both included.  From the goal, step to the first neighbour n in R1's order
 *      such that the move is legal and field[n] + w == field[here]; stop at value 0; the cells are emitted reversed.  A goal
 *      that is unreached, not passable or outside the image has an empty path -- and so has a goal from which some step finds
 *      no such neighbour (a field that R2 did not make).
 *  R6. The cell of a world coordinate is N6's rule 1, floor((v - pcd_min) / cell_size) in float64; the Python layer applies it.
 * hmsg_nav_route is the composition and only that: passable = the mask where clearance >= min_clearance (min_clearance 0: the
 * mask itself); the start is snapped with no field; one field is built from it; every goal is snapped among the reached cells;
 * the paths are extracted to the snapped cells.  Any pointer of hmsg_nav_routes may be NULL.  A path list that is too short
 * behaves as boundary_capacity does: everything else is written, the list is not, the count says what is needed
 * (HMSG_ERR_INVALID).  path_off / path_rc of hmsg_nav_paths may be NULL (the count alone); d2 and n_reached may be NULL.  The
 * structs themselves and n_needed are host memory; src_off and src_rc are read and checked by the host before anything runs.
 * Refusals (HMSG_ERR_INVALID unless said): a null required pointer; rows or cols < 1; w_straight < 1 or w_diag < w_straight;
 * min_clearance < 0; a decreasing src_off; a source with an index outside the image; HMSG_ERR_UNSUPPORTED when rows * cols >=
 * 2^28 or rows * cols * w_diag >= 2^31 (below these no finite value can overflow). */
#define HMSG_NAV_UNREACHED 2147483647
typedef struct hmsg_route_params {
    int32_t w_straight, w_diag;   /* 5, 7 */
    int32_t min_clearance;        /* 0; in field units; hmsg_nav_route alone reads it */
    int32_t reserved_;
} hmsg_route_params;
typedef struct hmsg_nav_routes {
    int32_t* goal_cell;           /* i32 [n_goals][2]: the snapped cell, (-1, -1) when nothing is reached */
    int64_t* goal_d2;             /* i64 [n_goals]: R4's d2 of the snap */
    int32_t* goal_dist;           /* i32 [n_goals]: the field at the snapped cell */
    int64_t* path_off;            /* i64 [n_goals + 1] */
    int32_t* path_rc;             /* i32 [path_capacity][2] */
    int64_t  path_capacity;
    int32_t* field;               /* i32 [rows][cols]: the start's field (optional, like the next) */
    uint8_t* passable;            /* u8 [rows][cols] */
    /* out */
    int64_t  n_path_cells;
    int64_t  start_d2;            /* R4's d2 of the start's snap; -1: no passable cell */
    int32_t  start_cell[2];
} hmsg_nav_routes;
void hmsg_route_default_params(hmsg_route_params* p);
int hmsg_nav_clearance(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* mask, const hmsg_route_params* prm, int32_t* clearance);
/* n_fields source sets in one call: the cells src_rc[src_off[s] .. src_off[s + 1]) are the sources of fields[s] */
int hmsg_nav_distance_fields(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* passable, const hmsg_route_params* prm,
                             int32_t n_fields, const int64_t* src_off /* [n_fields + 1] */, const int32_t* src_rc,
                             int32_t* fields /* [n_fields][rows][cols] */, int64_t* n_reached /* [n_fields], may be NULL */);
int hmsg_nav_snap_cells(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* passable, const int32_t* field /* or NULL */, int64_t n,
                        const int32_t* target_rc, int32_t* snapped_rc, int64_t* d2);
int hmsg_nav_paths(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* passable, const hmsg_route_params* prm, const int32_t* field,
                   int64_t n_goals, const int32_t* goal_rc, int64_t* path_off /* [n_goals + 1] */, int32_t* path_rc, int64_t capacity,
                   int64_t* n_needed);
int hmsg_nav_route(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* main_free_map, const hmsg_route_params* prm,
                   const int32_t* start_rc, int64_t n_goals, const int32_t* goal_rc, hmsg_nav_routes* out);

/* ---- N8: viewpoints on a floor's free map (csrc/hmsg_navview.hip): the cells from which a goal is in sight, and the one to stand
 * on.  R4 takes the nearest passable, reached cell whatever lies between it and the goal; with a clearance the passable set
 * shrinks away from every wall, and the nearest passable cell of an object in a narrow room or on a wall can be on the wall's
 * other side.  The reference has no such stage (goal_pose_publisher.py:260-271 publishes an object's centre; the slow path
 * matches the object again in the camera image on arrival), so the rules are this library's.  Images, cells and memory
 * conventions are N7's.  blocking is u8 [rows][cols], a cell is opaque where its byte is not 0 (a storey's obstacle_map);
 * passable is u8 [rows][cols]; field (optional) is an R2 field on passable.  All of it is integer work: every output has one
 * right answer.  The rules:
 *  V1. Sight line of the cells a and b: start from whichever of the two has the smaller (row, col) pair, so dr >= 0.  n =
 *      max(|dr|, |dc|).  For i = 0 .. n the major coordinate advances by one per step (towards the other cell) and the minor
 *      coordinate is m0 + floor((2 * i * dm + n) / (2 * n)) -- the mathematical floor, not C's truncation: dm may be negative.
 *      The major axis is the row axis when |dr| >= |dc|.  n = 0: the single cell.  The start is chosen by the cells, not by the
 *      caller: line(a, b) == line(b, a).
 *  V2. Clear sight: no cell of the line but its two endpoints is blocking, and no diagonal step of the line squeezes between
 *      two blocking cells -- for consecutive cells (r0, c0) -> (r1, c1) with both coordinates changing, blocking[r0][c1] &&
 *      blocking[r1][c0] blocks ([[1, 0], [0, 1]] is opaque, as in R1).  The endpoints never block: an object's centre may lie
 *      inside an obstacle.
 *  V3. Visible set of a goal g: the cells c of the image with passable[c] != 0; field[c] finite, when a field is given; r_min2
 *      <= d2(c, g) <= r_max2, d2 = dr * dr + dc * dc in int64; and a clear sight from c to g.  A goal outside the image has an
 *      empty set.
 *  V4. Viewpoint: the member of the visible set with the least key -- prefer 0 (least walk): (field value, d2, row-major index);
 *      prefer 1 (closest look): (d2, field value, row-major index).  Without a field the field value counts as 0 for every
 *      cell (and view_dist is 0).  An empty set gives the cell (-1, -1), d2 = -1 and dist = HMSG_NAV_UNREACHED.
 *  V5. Limits: r_max2 <= 255 * 255, so that the window round a goal is at most 511 x 511 cells and one workgroup holds its
 *      blocking bits in LDS.
 * hmsg_nav_viewpoints: n_visible[k] is the size of goal k's visible set and visible[k] its mask (1 / 0), every byte written;
 * view_d2, view_dist, n_visible and visible may each be NULL.  hmsg_nav_view_route is hmsg_nav_route with its goal snap (R4)
 * replaced by V4 on the start's field, and only that: the clearance -> passable step, the start's snap, the field, the paths,
 * the fields of hmsg_nav_routes and the too-short path list are hmsg_nav_route's; goal_cell is the viewpoint, goal_d2 its d2,
 * goal_dist its field value; n_visible (i32 [n_goals]) may be NULL.  Every array may be host or device memory; the structs are
 * host memory.  Refusals (HMSG_ERR_INVALID unless said): a null required pointer; rows or cols < 1; n_goals < 0; r_min2 < 0;
 * r_max2 < r_min2; prefer not 0 or 1; HMSG_ERR_UNSUPPORTED when r_max2 > 255 * 255 or rows * cols >= 2^28; for
 * hmsg_nav_view_route also hmsg_nav_route's. */
typedef struct hmsg_view_params {
    int64_t r_min2, r_max2;       /* 0, 100 * 100: the band of squared distances to the goal, in cells */
    int32_t prefer;               /* 0: least walk; 1: closest look */
    int32_t reserved_;
} hmsg_view_params;
void hmsg_view_default_params(hmsg_view_params* p);
int hmsg_nav_viewpoints(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* blocking, const uint8_t* passable,
                        const int32_t* field /* or NULL */, const hmsg_view_params* prm, int64_t n_goals, const int32_t* goal_rc,
                        int32_t* view_rc /* i32 [n_goals][2] */, int64_t* view_d2 /* i64 [n_goals] */, int32_t* view_dist /* i32 [n_goals] */,
                        int32_t* n_visible /* i32 [n_goals] */, uint8_t* visible /* u8 [n_goals][rows][cols] */);
int hmsg_nav_view_route(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* main_free_map, const uint8_t* blocking,
                        const hmsg_route_params* route_prm, const hmsg_view_params* view_prm, const int32_t* start_rc, int64_t n_goals,
                        const int32_t* goal_rc, hmsg_nav_routes* out, int32_t* n_visible /* i32 [n_goals], may be NULL */);

/* ---- N9: routes across storeys (csrc/hmsg_navbuilding.hip): exact fields over several maps that are joined at a few cells (stairs,
 * a lift), the goals' cells and the cells of the way through such joins.  The reference has no such stage (its global navigation
 * graph joins two floors by one Voronoi edge; goal_pose_publisher.py:260-271 publishes an object's centre), so the rules are this
 * library's.  Images, cells, weights and memory conventions are N7's; R1 to R6 hold on every storey.  All of it is integer work:
 * every output has one right answer.  The rules:
 *  B1. Seeded field: seeds are cells with an int32 cost >= 0.  field[c] = the minimum over the seeds s of cost_s + the least cost
 *      of a legal R1 walk from s to c.  A seed on a cell that is not passable is no seed; duplicate seeds on one cell count with
 *      their least cost; with no seed every cell is HMSG_NAV_UNREACHED.  hmsg_nav_distance_fields is the case of every cost 0.
 *  B2. Building: n_storeys maps, each with its own rows_l, cols_l and passable_l, and n_links links (storey_a, cell_a, storey_b,
 *      cell_b, cost), cost >= 1, written as seven int32: sa, ra, ca, sb, rb, cb, cost.  A link is walked in both directions at
 *      that cost.  A link with an endpoint on a cell that is not passable does not exist.  storey_a == storey_b is allowed (a
 *      lift, a door the map does not show).  The building's graph is the disjoint union of the storeys' R1 grid graphs plus the
 *      links.
 *  B3. Building field: for a start (storey, cell), field_l[c] = the least cost in that graph from the start to cell c of storey
 *      l, for every storey l.  A storey that no chain of links reaches is all unreached; a start on a cell that is not passable
 *      gives all-unreached fields everywhere.  n_reached counts the finite cells per start and per storey.
 *  B4. Goal: a goal is (storey, cell); its snap is R4 on its own storey among the cells whose building field is finite.  No
 *      candidate on that storey: cell (-1, -1), d2 = -1, dist = HMSG_NAV_UNREACHED.
 *  B5. Path: (storey, row, col) triples from the start to the goal, both included, emitted reversed as in R5.  From the goal, first
 *      R5's step on the same storey: the first neighbour in R1's order whose move is legal and whose field + w equals the value
 *      here.  If there is none, step through the first link in index order that exists (B2), has an endpoint here and whose other
 *      endpoint o has field[o] + cost == the value here; for one link the walk a -> b (here is b, o is a) is tried before b -> a.
 *      Stop at value 0.  If neither step exists the path is empty, as it is for a goal that is unreached, not passable or outside
 *      its image.  Every step lowers the value by at least 1, so the walk ends.
 *  B6. Limits: 1 <= n_storeys <= 256, 0 <= n_links < 2^20, every storey within N7's shape limits.  HMSG_ERR_UNSUPPORTED when
 *      w_diag * (the sum of rows_l * cols_l) + (the sum of the links' costs) reaches 2^31; for B1 when max seed cost + rows * cols *
 *      w_diag does.  Below these bounds no finite value overflows.  Refused with HMSG_ERR_INVALID: a link, start or goal with a
 *      storey index out of range; a link endpoint, seed or start with a cell index outside its image (the starts of
 *      hmsg_nav_building_fields: hmsg_nav_building_route snaps its start, whose cell may lie anywhere, as a goal's may); a cost
 *      < 1 of a link or < 0 of a seed; a null required pointer; N7's refusals of the weights.
 * Every array may be host or device memory; the structs and the arrays of pointers (rows, cols, passable, fields) are host
 * memory; links, seeds, starts and goals are read and checked by the host before anything runs.  n_reached, path_off, path_src
 * and every pointer of hmsg_nav_building_routes may be NULL as N7's may; a path list that is too short behaves as in
 * hmsg_nav_route.  hmsg_nav_building_route is the composition and only that: per storey passable = main_free_map where its
 * clearance reaches min_clearance, exactly as hmsg_nav_route does it; the start (storey, cell) is snapped by R4 on its storey
 * with no field; B3 for that one start; B4 per goal; B5 to the snapped cells.  With one storey and no link every output equals
 * hmsg_nav_route's, the triples carrying storey 0. */
typedef struct hmsg_nav_building_routes {
    int32_t* goal_cell;           /* i32 [n_goals][3]: the goal's storey and its snapped cell, (-1, -1) when nothing is reached there */
    int64_t* goal_d2;             /* i64 [n_goals] */
    int32_t* goal_dist;           /* i32 [n_goals]: the building field at the snapped cell */
    int64_t* path_off;            /* i64 [n_goals + 1] */
    int32_t* path_src;            /* i32 [path_capacity][3]: storey, row, col */
    int64_t  path_capacity;
    int32_t** field;              /* NULL, or n_storeys pointers (each NULL or i32 [rows_l][cols_l]): the start's building field */
    uint8_t** passable;           /* NULL, or n_storeys pointers (each NULL or u8 [rows_l][cols_l]) */
    /* out */
    int64_t  n_path_cells;
    int64_t  start_d2;            /* R4's d2 of the start's snap; -1: no passable cell on its storey */
    int32_t  start_cell[3];       /* storey, row, col */
    int32_t  reserved_;
} hmsg_nav_building_routes;
/* B1, batched like hmsg_nav_distance_fields: the seeds seed_rc / seed_cost [seed_off[s] .. seed_off[s + 1]) make fields[s] */
int hmsg_nav_seeded_fields(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* passable, const hmsg_route_params* prm,
                           int32_t n_fields, const int64_t* seed_off /* [n_fields + 1] */, const int32_t* seed_rc /* [m][2] */,
                           const int32_t* seed_cost /* [m] */, int32_t* fields /* [n_fields][rows][cols] */,
                           int64_t* n_reached /* [n_fields], may be NULL */);
/* B3 for n_starts starts in one call */
int hmsg_nav_building_fields(int32_t device_id, int32_t n_storeys, const int32_t* rows, const int32_t* cols,
                             const uint8_t* const* passable /* n_storeys pointers */, int32_t n_links,
                             const int32_t* links /* i32 [n_links][7]: sa, ra, ca, sb, rb, cb, cost */, const hmsg_route_params* prm,
                             int32_t n_starts, const int32_t* start /* i32 [n_starts][3]: storey, row, col */,
                             int32_t* const* fields /* one pointer per storey: i32 [n_starts][rows_l][cols_l] */,
                             int64_t* n_reached /* i64 [n_starts][n_storeys], may be NULL */);
/* B5 on the building field of one start (fields: one pointer per storey, i32 [rows_l][cols_l]) */
int hmsg_nav_building_paths(int32_t device_id, int32_t n_storeys, const int32_t* rows, const int32_t* cols, const uint8_t* const* passable,
                            int32_t n_links, const int32_t* links, const hmsg_route_params* prm, const int32_t* const* fields,
                            int64_t n_goals, const int32_t* goals /* i32 [n_goals][3] */, int64_t* path_off /* [n_goals + 1] */,
                            int32_t* path_src /* i32 [capacity][3] */, int64_t capacity, int64_t* n_needed);
int hmsg_nav_building_route(int32_t device_id, int32_t n_storeys, const int32_t* rows, const int32_t* cols,
                            const uint8_t* const* main_free_map /* n_storeys pointers */, int32_t n_links, const int32_t* links,
                            const hmsg_route_params* prm, const int32_t* start /* i32 [3] */, int64_t n_goals,
                            const int32_t* goals /* i32 [n_goals][3] */, hmsg_nav_building_routes* out);

/* ---- N10: sight over furniture (csrc/hmsg_navmap.hip, csrc/hmsg_navview.hip): an exact integer height map of a storey and N8's
 * sight rule in 2.5-D on top of it.  N8 judges sight on obstacle_map > 0, a flat image of the points between obstacle_lo and
 * obstacle_hi: nothing below that band hides anything, and with the band lowered a table hides a lamp as a wall does.  The
 * reference's get_height_map is last-writer-wins in float and feeds an older stairs variant only; it is not restated, and the
 * rules are this library's.  Images, cells and memory conventions are N6's and N7's.  All of it is integer work: every output has
 * one right answer.
 * The height map:
 *  H1. The grid (pcd_min, pcd_max, grid) is N6's rule 1 over ALL points of the storey, so the map lies cell for cell on the maps
 *      hmsg_nav_floor_maps makes of the same cloud.  A point takes part when y < zero_level + top_max (the sum formed in float64
 *      first, as in N6's rule 2; top_max keeps ceilings out).  Its cell is N6's rule 1 for x and z; its height is q = floor((y -
 *      zero_level) / height_unit) in float64 (subtract, then divide), clamped to [0, 65535].
 *  H2. raw[cell] = the maximum q of the cell's points, 0 for a cell with none; known[cell] (u8) = 1 where a point took part.
 *  H3. top[cell] (u16) = the maximum of raw over the dilation x dilation box centred on the cell, clipped at the image border.
 *      dilation is odd (5, as the obstacle map's: the map's voxels are coarser than the cells, and without it a wall is a
 *      sieve); 0 or 1: top = raw.
 * Refusals: N6's (a null prm / xyz / top, no points, a coordinate that is not finite, counted on the device; HMSG_ERR_UNSUPPORTED
 * for a grid of 2^28 cells or more); height_unit <= 0, top_max <= 0, cell_size <= 0, a dilation outside [0, 63];
 * HMSG_ERR_UNSUPPORTED for an even dilation other than 0.  known may be NULL; pcd_min, pcd_max and grid may be NULL.  The graph
 * and scene forms take the slabs of their _floor_maps siblings and refuse what those refuse.
 * Sight with heights: eye is the camera's height above the storey's zero level in height units, one value per call; goal_h[k]
 * (i32, read clamped to [0, 65535]) is goal k's height, goal_r2[k] (i64; the array may be NULL: -1 everywhere) its footprint.
 *  S1. The line of two cells is V1, unchanged: it starts at the smaller (row, col) pair, indices i = 0 .. n.  Each end keeps its
 *      height: the viewpoint's end eye, the goal's end goal_h.  h0 is the height at i = 0, hn the one at i = n.
 *  S2. T(c) = 0 when d2(c, goal) <= goal_r2, else top[c]: the object's own body does not hide its centre.  The sight is clear
 *      when no cell 0 < i < n has T(c_i) * n >= h0 * (n - i) + hn * i, and no diagonal step i - 1 -> i has BOTH cells s it
 *      squeezes between at T(s) * 2 n >= h0 * (2 n - 2 i + 1) + hn * (2 i - 1).  The endpoints never block.  Every product fits
 *      int32 (65535 * 510).  A column is solid from the floor to its top: there is no seeing under a table.
 *  S3. The visible set is V3 with S2 in V2's place.
 *  S4. The viewpoint is V4, unchanged.
 *  S5. Limits are V5's.  Refusals are N8's, plus eye outside [0, 65535], a goal_r2[k] < -1, a null top or goal_h.
 * With top = 65535 where a cell blocks and 0 elsewhere, no footprint and eye and goal_h anywhere in [1, 65535], S3 is V3 bit for
 * bit.  hmsg_nav_view_route_h is hmsg_nav_view_route with S3 in V3's place, and only that. */
typedef struct hmsg_height_params {
    double  cell_size;            /* 0.03 m */
    double  height_unit;          /* 0.01 m */
    double  top_max;              /* 2.5: points at zero_level + top_max and above take no part */
    int32_t dilation;             /* 5; odd; 0 or 1 = none */
    int32_t reserved_;
} hmsg_height_params;
void hmsg_height_default_params(hmsg_height_params* p);
/* xyz f64 [n][3]; top u16 [grid[1]][grid[0]], known u8 of the same shape or NULL (hmsg_nav_grid says the size beforehand) */
int hmsg_nav_height_map(int32_t device_id, const hmsg_height_params* prm, int64_t n, const double* xyz, double zero_level, uint16_t* top,
                        uint8_t* known, double* pcd_min /* f64 [3] */, double* pcd_max, int32_t* grid /* i32 [2] */);
int hmsg_graph_nav_height_map(hmsg_graph_t* g, int32_t floor, const hmsg_height_params* prm, uint16_t* top, uint8_t* known, double* pcd_min,
                              double* pcd_max, int32_t* grid);
int hmsg_map_nav_height_map(hmsg_t* h, double y_lo, double y_hi, double zero_level, const hmsg_height_params* prm, uint16_t* top,
                            uint8_t* known, double* pcd_min, double* pcd_max, int32_t* grid);
int hmsg_nav_viewpoints_h(int32_t device_id, int32_t rows, int32_t cols, const uint16_t* top, const uint8_t* passable,
                          const int32_t* field /* or NULL */, const hmsg_view_params* prm, int32_t eye, int64_t n_goals, const int32_t* goal_rc,
                          const int32_t* goal_h /* i32 [n_goals] */, const int64_t* goal_r2 /* i64 [n_goals] or NULL */, int32_t* view_rc,
                          int64_t* view_d2, int32_t* view_dist, int32_t* n_visible, uint8_t* visible);
int hmsg_nav_view_route_h(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* main_free_map, const uint16_t* top,
                          const hmsg_route_params* route_prm, const hmsg_view_params* view_prm, int32_t eye, const int32_t* start_rc,
                          int64_t n_goals, const int32_t* goal_rc, const int32_t* goal_h, const int64_t* goal_r2 /* or NULL */,
                          hmsg_nav_routes* out, int32_t* n_visible /* i32 [n_goals], may be NULL */);

/* ---- N11: rooms on a floor's free map (csrc/hmsg_navrooms.hip): every reached cell gets a room, the cells where two rooms touch
 * become doors, a way is cut into legs by room.  The scene graph has rooms as clouds and (x, z) vertices, N6 to N10 have a map
 * whose cells belong to no room; the reference joins the two nowhere (its graph has no room-room edge, its navigation graph knows
 * no rooms), so the rules are this library's.  Images, cells, weights and memory conventions are N7's; R1 to R6 hold.  passable is
 * u8 [rows][cols].  The rooms' seeds are cells seed_rc i32 [sum][2] with the CSR offsets seed_off i64 [n_rooms + 1]: room r is
 * seeded by seed_rc[seed_off[r] .. seed_off[r + 1]).  The Python layer makes the seeds from room.vertices by R6.  All of it is
 * integer work: every output has one right answer.  The rules:
 *  G1. Room field: dist is R2's field from the union of all rooms' seed cells.  A seed on a cell that is not passable is no
 *      source.  Duplicate seeds are fine, within a room and between rooms.
 *  G2. Label: label[c] is the least room index r such that R2's field from room r's seeds alone equals dist[c] at c; -1 where
 *      dist[c] is HMSG_NAV_UNREACHED, which includes every cell that is not passable.  Labels are int32.  A room without a passable
 *      seed labels no cell.  n_cells[r] (int64) counts the cells of label r.  Equivalent form: the label of a source cell is the
 *      least room that seeds it, and label[c] = min label[n] over R1-legal moves n -> c with dist[n] + w == dist[c].  (Min over
 *      tight predecessors, by induction on dist, is the least room that has a shortest walk to c.)
 *  D1. Border move: an R1-legal move between cells a and b with label[a] >= 0, label[b] >= 0 and label[a] != label[b].  The
 *      corner rule applies: [[1, 0], [0, 1]] is no contact.
 *  D2. Threshold cell: other[a] is the least label[b] over a's border moves, -1 where a has none; int32 [rows][cols].  A threshold
 *      cell has other >= 0; its pair is (min(label, other), max(label, other)).  Every threshold cell has exactly one pair.
 *  D3. Door: a connected component of the threshold cells of equal pair, by the plain 8-neighbourhood inside the image (no corner
 *      rule here: scipy.ndimage.label with a 3 x 3 structure restates it).
 *  D4. Door table: the doors sorted by (p, q, least row-major index of the door's cells).  door_pair i32 [n_doors][2]; door_off
 *      i64 [n_doors + 1]; door_rc i32 [n_door_cells][2], each door's cells in ascending row-major order.  A door's middle is the
 *      cell at position floor((n - 1) / 2) of its list; the Python layer takes it.  adjacency i32 [n_rooms][n_rooms], optional:
 *      the number of doors of each pair, symmetric with a zero diagonal.
 *  L1. Legs of a way: for a path list as hmsg_nav_paths gives it (path_off, path_rc), the run-length of label along each path:
 *      leg_off i64 [n_paths + 1], leg_room i32, leg_first i64 (the index within its path of a leg's first cell).  A path cell
 *      outside the image has label -1.  An empty path has no leg.
 * hmsg_nav_room_doors is the composition and only that: passable as hmsg_nav_route makes it (the mask where clearance >=
 * min_clearance), the labels, the doors, with nothing leaving the device between them.  Every array may be host or device memory;
 * structs and counts are host memory; seed_off, seed_rc and path_off are read and checked by the host before anything runs.  Any
 * pointer of hmsg_nav_door_table may be NULL.  A list that is too short behaves as path_rc does in N7: everything else is written,
 * the list is not, the counts say what is needed (HMSG_ERR_INVALID); door_capacity speaks for door_pair and door_off, cell_capacity
 * for door_rc, capacity for leg_room and leg_first (which come together or not at all).  dist, n_cells, leg_off and passable (of
 * hmsg_nav_room_doors) may be NULL.
 * Refusals (HMSG_ERR_INVALID unless said): a null required pointer; rows or cols < 1; n_rooms < 0 or n_paths < 0; a negative
 * capacity; a decreasing offset array; a seed outside the image; a label >= n_rooms or < -1 in the label image handed to
 * hmsg_nav_doors (checked on the device, reported after the call); N7's refusals of the weights and min_clearance;
 * HMSG_ERR_UNSUPPORTED for N7's size limits and for adjacency with n_rooms > 4096. */
typedef struct hmsg_nav_door_table {
    int32_t* door_pair;           /* i32 [door_capacity][2] */
    int64_t* door_off;            /* i64 [door_capacity + 1] */
    int32_t* door_rc;             /* i32 [cell_capacity][2] */
    int32_t* other;               /* i32 [rows][cols] */
    int32_t* adjacency;           /* i32 [n_rooms][n_rooms] */
    int64_t  door_capacity, cell_capacity;
    /* out */
    int64_t  n_doors, n_door_cells;
} hmsg_nav_door_table;
int hmsg_nav_room_labels(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* passable, const hmsg_route_params* prm, int32_t n_rooms,
                         const int64_t* seed_off /* [n_rooms + 1] */, const int32_t* seed_rc, int32_t* label /* [rows][cols] */,
                         int32_t* dist /* [rows][cols] or NULL */, int64_t* n_cells /* [n_rooms] or NULL */);
int hmsg_nav_doors(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* passable, const int32_t* label, int32_t n_rooms,
                   hmsg_nav_door_table* out);
int hmsg_nav_path_rooms(int32_t device_id, int32_t rows, int32_t cols, const int32_t* label, int64_t n_paths, const int64_t* path_off,
                        const int32_t* path_rc, int64_t* leg_off /* [n_paths + 1] */, int32_t* leg_room, int64_t* leg_first, int64_t capacity,
                        int64_t* n_needed);
int hmsg_nav_room_doors(int32_t device_id, int32_t rows, int32_t cols, const uint8_t* main_free_map, const hmsg_route_params* prm,
                        int32_t n_rooms, const int64_t* seed_off, const int32_t* seed_rc, int32_t* label, uint8_t* passable /* or NULL */,
                        hmsg_nav_door_table* out);


#ifdef __cplusplus
}
#endif
#endif /* HMSG_H */
