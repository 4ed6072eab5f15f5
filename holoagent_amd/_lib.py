"""ctypes binding of the C ABI in include/hmsg.h.

The product path loads ONLY `holoagent_amd/libhmsg.so` (hand-written HIP for gfx950, built by
`__graft_entry__.build()` / `make -C holoagent_amd/csrc`) and raises if it is missing -- there is no
CPU fallback.  (`HmsgLib(path)` with an explicit path exists so the test-suite can drive the kernel
simulator build of the same sources, tests/emu/.)
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhmsg.so")


class HmsgConfig(C.Structure):
    _fields_ = [
        ("device_id", C.c_int32), ("feat_dim", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
        ("max_frames", C.c_int32), ("max_masks", C.c_int32),
        ("voxel_size", C.c_double), ("depth_scale", C.c_double), ("init_overlap_thresh", C.c_double),
        ("overlap_thresh_factor", C.c_double), ("iou_thresh", C.c_double), ("clip_masked_weight", C.c_double),
        ("max_mask_distance", C.c_double), ("merge_type", C.c_int32), ("outlier_nb_points", C.c_int32),
        ("outlier_radius", C.c_double), ("pool_max_dist", C.c_double), ("feat_dbscan_eps", C.c_double),
        ("feat_dbscan_min", C.c_int32), ("merge_dbscan_eps", C.c_double), ("merge_dbscan_min", C.c_int32),
        ("min_instance_points", C.c_int32), ("skip_frames", C.c_int32), ("depth_cut", C.c_double), ("grid_resolution", C.c_double),
        ("overlap_distance_form", C.c_int32),
    ]


class HmsgNode(C.Structure):          # include/hmsg.h: hmsg_node
    _fields_ = [("instance", C.c_int32), ("floor", C.c_int32), ("room", C.c_int32), ("counter", C.c_int32),
                ("label", C.c_int32), ("n_points", C.c_int64)]


class HmsgDepthParams(C.Structure):    # include/hmsg.h: hmsg_depth_params
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("image_scale", C.c_int32), ("fx", C.c_double),
                ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("voxel_size", C.c_double),
                ("depth_factor", C.c_double)]


class HmsgObjectRecord(C.Structure):   # include/hmsg.h: hmsg_object_record
    _fields_ = [("instance", C.c_int32), ("file_stem", C.c_char_p), ("object_id_json", C.c_char_p),
                ("room_id_json", C.c_char_p), ("name_json", C.c_char_p), ("view_ids_json", C.c_char_p),
                ("best_view_id_json", C.c_char_p)]


class HmsgJsonField(C.Structure):      # include/hmsg.h: hmsg_json_field
    _fields_ = [("key", C.c_char_p), ("kind", C.c_int32), ("ndim", C.c_int32), ("n0", C.c_int64), ("n1", C.c_int64), ("data", C.c_void_p)]


class HmsgGraphParams(C.Structure):    # include/hmsg.h: hmsg_graph_params
    _fields_ = [("num_views", C.c_int32), ("kmeans_n_init", C.c_int32), ("kmeans_max_iter", C.c_int32), ("kmeans_seed", C.c_uint32),
                ("skip_frames", C.c_int32), ("image_width", C.c_int32), ("image_height", C.c_int32), ("min_visible_ratio", C.c_double),
                ("max_view_depth", C.c_double), ("host_threads", C.c_int32), ("merge_objects_graph", C.c_int32), ("kmeans_device", C.c_int32)]


class HmsgGraphCounts(C.Structure):    # include/hmsg.h: hmsg_graph_counts
    _fields_ = [("floors", C.c_int32), ("rooms", C.c_int32), ("views", C.c_int32), ("objects", C.c_int32), ("edges", C.c_int64),
                ("view_object_links", C.c_int64), ("begin_ms", C.c_double), ("finish_ms", C.c_double), ("kmeans_wait_ms", C.c_double)]


class HmsgGraphObject(C.Structure):    # include/hmsg.h: hmsg_graph_object
    _fields_ = [("object_id", C.c_char * 48), ("name", C.c_char * 80), ("room", C.c_int32), ("instance", C.c_int32), ("label", C.c_int32),
                ("n_views", C.c_int32), ("best_view", C.c_int32)]


class HmsgGraphRoom(C.Structure):      # include/hmsg.h: hmsg_graph_room
    _fields_ = [("room_id", C.c_char * 32), ("name", C.c_char * 80), ("floor", C.c_int32), ("n_vertices", C.c_int64), ("n_points", C.c_int64),
                ("n_embeddings", C.c_int32), ("n_sample_images", C.c_int32), ("n_objects", C.c_int32), ("n_views", C.c_int32)]


class HmsgGraphView(C.Structure):      # include/hmsg.h: hmsg_graph_view
    _fields_ = [("view", C.c_int32), ("room", C.c_int32), ("img_id", C.c_int64), ("n_objects", C.c_int32), ("reserved_", C.c_int32)]


class HmsgClipPreprocess(C.Structure):   # include/hmsg.h: hmsg_clip_preprocess
    _fields_ = [("size", C.c_int32), ("out_f16", C.c_int32), ("mean", C.c_float * 3), ("std", C.c_float * 3)]


class HmsgSamPostParams(C.Structure):   # include/hmsg.h: hmsg_sam_post_params
    _fields_ = [("pred_iou_thresh", C.c_float), ("stability_score_thresh", C.c_float), ("stability_score_offset", C.c_float),
                ("mask_threshold", C.c_float), ("box_nms_thresh", C.c_float), ("min_mask_region_area", C.c_int32)]


class HmsgNavParams(C.Structure):       # include/hmsg.h: hmsg_nav_params
    _fields_ = [("cell_size", C.c_double), ("obstacle_lo", C.c_double), ("obstacle_hi", C.c_double), ("region_max", C.c_double),
                ("pose_radius", C.c_double), ("pose_eps", C.c_double), ("dilation", C.c_int32), ("blur", C.c_int32),
                ("pose_min_samples", C.c_int32), ("region_rule", C.c_int32)]


class HmsgNavMaps(C.Structure):         # include/hmsg.h: hmsg_nav_maps
    _fields_ = [("obstacle_map", C.c_void_p), ("region_map", C.c_void_p), ("poses_map", C.c_void_p), ("free_map", C.c_void_p),
                ("main_free_map", C.c_void_p), ("top_down_bgr", C.c_void_p), ("boundary_rc", C.c_void_p), ("boundary_capacity", C.c_int64),
                ("n_boundary", C.c_int64), ("main_area", C.c_int64), ("n_regions", C.c_int32), ("main_label", C.c_int32),
                ("grid", C.c_int32 * 2), ("pcd_min", C.c_double * 3), ("pcd_max", C.c_double * 3)]


class HmsgRouteParams(C.Structure):     # include/hmsg.h: hmsg_route_params
    _fields_ = [("w_straight", C.c_int32), ("w_diag", C.c_int32), ("min_clearance", C.c_int32), ("reserved_", C.c_int32)]


class HmsgNavRoutes(C.Structure):       # include/hmsg.h: hmsg_nav_routes
    _fields_ = [("goal_cell", C.c_void_p), ("goal_d2", C.c_void_p), ("goal_dist", C.c_void_p), ("path_off", C.c_void_p),
                ("path_rc", C.c_void_p), ("path_capacity", C.c_int64), ("field", C.c_void_p), ("passable", C.c_void_p),
                ("n_path_cells", C.c_int64), ("start_d2", C.c_int64), ("start_cell", C.c_int32 * 2)]


class HmsgNavBuildingRoutes(C.Structure):       # include/hmsg.h: hmsg_nav_building_routes
    _fields_ = [("goal_cell", C.c_void_p), ("goal_d2", C.c_void_p), ("goal_dist", C.c_void_p), ("path_off", C.c_void_p),
                ("path_src", C.c_void_p), ("path_capacity", C.c_int64), ("field", C.POINTER(C.c_void_p)), ("passable", C.POINTER(C.c_void_p)),
                ("n_path_cells", C.c_int64), ("start_d2", C.c_int64), ("start_cell", C.c_int32 * 3), ("reserved_", C.c_int32)]


class HmsgNavDoorTable(C.Structure):    # include/hmsg.h: hmsg_nav_door_table
    _fields_ = [("door_pair", C.c_void_p), ("door_off", C.c_void_p), ("door_rc", C.c_void_p), ("other", C.c_void_p), ("adjacency", C.c_void_p),
                ("door_capacity", C.c_int64), ("cell_capacity", C.c_int64), ("n_doors", C.c_int64), ("n_door_cells", C.c_int64)]


class HmsgViewParams(C.Structure):      # include/hmsg.h: hmsg_view_params
    _fields_ = [("r_min2", C.c_int64), ("r_max2", C.c_int64), ("prefer", C.c_int32), ("reserved_", C.c_int32)]


class HmsgHeightParams(C.Structure):    # include/hmsg.h: hmsg_height_params
    _fields_ = [("cell_size", C.c_double), ("height_unit", C.c_double), ("top_max", C.c_double), ("dilation", C.c_int32), ("reserved_", C.c_int32)]


class HmsgError(RuntimeError):
    pass


_P = C.c_void_p
_SIGS = {
    "hmsg_default_config": (None, [C.POINTER(HmsgConfig)]),
    "hmsg_config_size": (C.c_size_t, []),
    "hmsg_create": (C.c_int, [C.POINTER(HmsgConfig), C.POINTER(_P)]),
    "hmsg_destroy": (None, [_P]),
    "hmsg_last_error": (C.c_char_p, [_P]),
    "hmsg_version": (C.c_char_p, []),
    "hmsg_release_cached_memory": (None, []),
    "hmsg_reset": (C.c_int, [_P]),
    "hmsg_set_profiling": (C.c_int, [_P, C.c_int32]),
    "hmsg_profile_count": (C.c_int32, [_P]),
    "hmsg_profile_entry": (C.c_int, [_P, C.c_int32, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double)]),
    "hmsg_synth_render": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P,
                                    C.c_int32, _P, _P, C.c_double, C.c_uint64, _P, _P, _P, _P]),
    "hmsg_add_frames": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    "hmsg_finalize_map": (C.c_int, [_P]),
    "hmsg_map_size": (C.c_int64, [_P]),
    "hmsg_num_tie_queries": (C.c_int64, [_P]),
    "hmsg_map_size_unfiltered": (C.c_int64, [_P]),
    "hmsg_get_map_points": (C.c_int, [_P, _P, _P]),
    "hmsg_add_frame_features": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "hmsg_add_frame_features_rle": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "hmsg_rle_to_bitsets": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "hmsg_rle_to_masks": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "hmsg_sam_post_default_params": (None, [_P]),
    "hmsg_sam_postprocess": (C.c_int, [C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int64, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int64), _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_double)]),
    "hmsg_nav_default_params": (None, [_P]),
    "hmsg_nav_grid": (C.c_int, [C.c_int32, C.c_double, C.c_int64, _P, _P, _P, _P]),
    "hmsg_nav_floor_maps": (C.c_int, [C.c_int32, _P, C.c_int64, _P, _P, C.c_double, C.c_int32, _P, _P]),
    "hmsg_map_nav_grid": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, _P, _P, _P]),
    "hmsg_map_nav_floor_maps": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, _P, C.c_int32, _P, _P]),
    "hmsg_graph_nav_grid": (C.c_int, [_P, C.c_int32, C.c_double, _P, _P, _P]),
    "hmsg_graph_nav_floor_maps": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P]),
    "hmsg_route_default_params": (None, [_P]),
    "hmsg_nav_clearance": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "hmsg_nav_distance_fields": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P]),
    "hmsg_nav_snap_cells": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int64, _P, _P, _P]),
    "hmsg_nav_paths": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "hmsg_nav_route": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int64, _P, _P]),
    "hmsg_view_default_params": (None, [_P]),
    "hmsg_nav_viewpoints": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "hmsg_nav_view_route": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int64, _P, _P, _P]),
    "hmsg_height_default_params": (None, [_P]),
    "hmsg_nav_height_map": (C.c_int, [C.c_int32, _P, C.c_int64, _P, C.c_double, _P, _P, _P, _P, _P]),
    "hmsg_graph_nav_height_map": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "hmsg_map_nav_height_map": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P, _P, _P]),
    "hmsg_nav_viewpoints_h": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P]),
    "hmsg_nav_view_route_h": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, C.c_int64, _P, _P, _P, _P, _P]),
    "hmsg_test_nav_sight_layout": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "hmsg_get_frame_num_masks": (C.c_int32, [_P, C.c_int32]),
    "hmsg_fuse_frames": (C.c_int, [_P]),
    "hmsg_get_map_feats": (C.c_int, [_P, _P, _P]),
    "hmsg_get_feature_sums": (C.c_int, [_P, _P, _P]),
    "hmsg_set_feature_sums": (C.c_int, [_P, _P, _P]),
    "hmsg_get_frame_nn": (C.c_int, [_P, C.c_int32, _P]),
    "hmsg_get_frame_fp": (C.c_int, [_P, C.c_int32, _P]),
    "hmsg_get_frame_mask_sizes": (C.c_int, [_P, C.c_int32, _P]),
    "hmsg_get_frame_mask_points": (C.c_int, [_P, C.c_int32, _P]),
    "hmsg_merge_instances": (C.c_int, [_P]),
    "hmsg_set_frame_window": (C.c_int, [_P, C.c_int32]),
    "hmsg_set_merge_tree_batch": (C.c_int, [_P, C.c_int64]),
    "hmsg_merge_tree_local": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "hmsg_merge_tree_join": (C.c_int, [_P, C.c_int32, _P, _P, C.c_double, C.c_int32]),
    "hmsg_num_instances": (C.c_int64, [_P]),
    "hmsg_get_instance_sizes": (C.c_int, [_P, _P]),
    "hmsg_get_instance_points": (C.c_int, [_P, _P]),
    "hmsg_get_instance_boxes": (C.c_int, [_P, _P]),
    "hmsg_denoise_instances": (C.c_int, [_P, C.c_double, C.c_int32]),
    "hmsg_instance_room_share": (C.c_int, [_P, C.c_int32, _P, _P, C.c_double, _P]),
    "hmsg_voxel_down_sample": (C.c_int, [_P, _P, C.c_int64, C.c_double, _P, _P]),
    "hmsg_pool_instances": (C.c_int, [_P]),
    "hmsg_get_instance_feats": (C.c_int, [_P, _P]),
    "hmsg_restore_stage": (C.c_int, [_P, C.c_int64, _P, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "hmsg_read_ply": (C.c_int, [C.c_char_p, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "hmsg_build_object_nodes": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, C.c_int32, _P]),
    "hmsg_num_nodes": (C.c_int64, [_P]),
    "hmsg_get_nodes": (C.c_int, [_P, _P, _P]),
    "hmsg_index_from_nodes": (C.c_int, [_P, C.POINTER(_P)]),
    "hmsg_room_clouds": (C.c_int, [_P, C.c_double, C.c_double, _P, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "hmsg_graph_default_params": (None, [C.POINTER(HmsgGraphParams)]),
    "hmsg_build_graph": (C.c_int, [_P, C.POINTER(HmsgGraphParams), C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P, C.POINTER(_P)]),
    "hmsg_graph_begin": (C.c_int, [_P, C.POINTER(HmsgGraphParams), C.c_int32, _P, _P, _P, _P, C.POINTER(_P)]),
    "hmsg_graph_finish": (C.c_int, [_P, C.c_int32, _P, _P]),
    "hmsg_graph_destroy": (None, [_P]),
    "hmsg_graph_last_error": (C.c_char_p, [_P]),
    "hmsg_graph_get_counts": (C.c_int, [_P, C.POINTER(HmsgGraphCounts)]),
    "hmsg_graph_get_edges": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "hmsg_graph_get_objects": (C.c_int, [_P, _P, C.c_int64]),
    "hmsg_graph_get_rooms": (C.c_int, [_P, _P, C.c_int64]),
    "hmsg_graph_get_room_vertices": (C.c_int, [_P, C.c_int32, _P, C.c_int64]),
    "hmsg_graph_get_room_embeddings": (C.c_int, [_P, C.c_int32, _P, C.c_int64]),
    "hmsg_graph_to_json": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "hmsg_save": (C.c_int, [_P, C.c_char_p]),
    "hmsg_load": (C.c_int, [C.c_char_p, C.c_int32, C.POINTER(_P)]),
    "hmsg_graph_index": (C.c_int, [_P, _P, C.POINTER(_P)]),
    "hmsg_graph_query": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "hmsg_graph_get_views": (C.c_int, [_P, _P, C.c_int64]),
    "hmsg_graph_get_view_objects": (C.c_int, [_P, C.c_int32, _P, C.c_int64]),
    "hmsg_graph_find_view": (C.c_int, [_P, C.c_char_p, C.c_int64, C.POINTER(C.c_int32)]),
    "hmsg_graph_object_best_views": (C.c_int, [_P, C.c_int32, _P, _P, _P]),
    "hmsg_graph_goal_views": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P]),
    "hmsg_graph_rematch_in_views": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "hmsg_graph_object_view_depths": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "hmsg_index_set_views": (C.c_int, [_P, C.c_int64, _P, _P]),
    "hmsg_rematch_in_views": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    "hmsg_points_view_depths": (C.c_int, [C.c_int32, C.c_int64, _P, _P, _P, _P, _P, C.c_double, C.c_double, _P, _P, _P]),
    "hmsg_graph_name_rooms": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P]),
    "hmsg_graph_set_room_names": (C.c_int, [_P, C.c_int32, _P]),
    "hmsg_denoise_feats_batch": (C.c_int, [C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_double, C.c_int32, _P, _P]),
    "hmsg_kmeans": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, _P, _P, _P, _P]),
    "hmsg_kmeans_batch": (C.c_int, [C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, _P, _P, _P, _P]),
    "hmsg_test_kmeans_lloyd": (C.c_int, [C.c_int32, C.c_int32, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "hmsg_room_camera_distances": (C.c_int, [_P, C.c_int32, C.c_int64, _P, _P]),
    "hmsg_object_views": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int64, _P, _P, C.c_double, C.c_double, _P, _P]),
    "hmsg_segment_floors": (C.c_int, [_P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    "hmsg_segment_rooms": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _P, C.c_int64, C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P]),
    "hmsg_points_min_dist_2d": (C.c_int, [C.c_int32, C.c_int32, _P, _P, C.c_int64, _P, _P]),
    "hmsg_lidar_depth": (C.c_int, [C.c_int32, _P, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "hmsg_crop_resize_batch": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, C.c_double, C.c_int32, _P, _P, _P]),
    "hmsg_clip_default_preprocess": (None, [_P]),
    "hmsg_clip_preprocess_batch": (C.c_int, [C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "hmsg_frame_encoder_inputs": (C.c_int, [C.c_int32, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, C.c_double, C.c_int32, _P, _P]),
    "hmsg_save_objects": (C.c_int, [_P, C.c_char_p, C.c_int64, _P, C.c_int32]),
    "hmsg_graph_allgather_index": (C.c_int, [_P, _P, _P, C.POINTER(_P), _P, _P, _P]),
    "hmsg_graph_query_sharded": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P,
                                           _P, _P, _P, _P, _P]),
    "hmsg_graphs_query": (C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P,
                                    _P, _P, _P, _P, _P]),
    "hmsg_comm_send": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32]),
    "hmsg_comm_recv": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32]),
    "hmsg_merge_tree_sharded": (C.c_int, [_P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    "hmsg_merge_room_objects": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_double, C.c_double, C.POINTER(C.c_int32), _P, _P, C.c_int32]),
    "hmsg_cloud_set_overlaps": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, _P, _P, C.c_int64, _P, C.c_double, _P]),
    "hmsg_cloud_set_overlaps_kd": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, _P, _P, C.c_int64, _P, C.c_double, _P]),
    "hmsg_eval_object_matrices": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, C.c_double, _P, _P, C.POINTER(C.c_int64)]),
    "hmsg_lsap": (C.c_int, [C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(C.c_int32)]),
    "hmsg_eval_rooms": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, _P, _P, C.c_double, C.c_double, _P, _P, _P,
                                  C.POINTER(C.c_int64)]),
    "hmsg_eval_semantic_ranks": (C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "hmsg_eval_floors": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P]),
    "hmsg_eval_metrics_from_matrix": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "hmsg_eval_counts_at": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_double, _P]),
    "hmsg_eval_hydra_means": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    "hmsg_eval_top_k": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P]),
    "hmsg_semseg_instance_labels": (C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "hmsg_knn_labels": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int32, _P, _P]),
    "hmsg_semseg_confusion": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int32, _P]),
    "hmsg_semseg_metrics": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P]),
    "hmsg_evaluate_semseg": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    "hmsg_eval_default_params": (None, [_P]),
    "hmsg_graph_evaluate": (C.c_int, [_P, _P, _P, _P, _P]),
    "hmsg_write_json": (C.c_int, [C.c_char_p, C.c_int32, _P]),
    "hmsg_write_ply": (C.c_int, [C.c_char_p, _P, C.c_int64]),
    "hmsg_read_json_numbers": (C.c_int, [C.c_char_p, C.c_char_p, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "hmsg_assign_cameras_to_rooms": (C.c_int, [_P, C.c_int64, C.c_int32, _P, C.c_double, C.c_double, _P, _P, _P]),
    "hmsg_pick_representative_views": (C.c_int, [_P, C.c_int64, C.c_int32, _P, _P, C.c_int32, _P, C.POINTER(C.c_int32)]),
    "hmsg_graph_edges": (C.c_int, [C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "hmsg_test_format_doubles": (C.c_int64, [_P, C.c_int64, _P, C.c_int64]),
    "hmsg_test_allocator_carving": (C.c_int, [C.c_int32, C.c_int32]),
    "hmsg_test_dbscan": (C.c_int, [_P, C.c_int32, _P, C.c_double, C.c_int32, _P, _P, _P, _P, _P]),
    "hmsg_index_load_objects": (C.c_int, [C.c_int32, C.c_char_p, C.c_int64, _P, _P, C.c_int32, C.POINTER(_P), C.POINTER(C.c_int32)]),
    "hmsg_index_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, _P, C.c_int32, _P, C.POINTER(_P)]),
    "hmsg_index_destroy": (None, [_P]),
    "hmsg_index_last_error": (C.c_char_p, [_P]),
    "hmsg_index_set_profiling": (C.c_int, [_P, C.c_int32]),
    "hmsg_index_profile": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "hmsg_query_objects": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "hmsg_similarity": (C.c_int, [_P, C.c_int32, _P, _P]),
    "hmsg_index_set_hierarchy": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "hmsg_query_hier": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "hmsg_comm_unique_id": (C.c_int, [_P]),
    "hmsg_comm_create": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    "hmsg_comm_destroy": (None, [_P]),
    "hmsg_comm_last_error": (C.c_char_p, [_P]),
    "hmsg_allgather_nodes": (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P), _P, _P]),
    "hmsg_allreduce_feature_sums": (C.c_int, [_P, _P]),
    "hmsg_test_sort_pairs": (C.c_int, [_P, _P, C.c_int64, C.c_int32]),
    "hmsg_test_repeat_add": (C.c_int, [_P, _P, _P, _P, C.c_int64]),
    "hmsg_test_ckdtree": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, _P, _P]),
    "hmsg_test_boundary": (C.c_int, [C.c_int32, _P, C.c_int64]),
    "hmsg_test_group_pairs": (C.c_int, [C.c_int32, C.c_int64, _P, C.c_int32, _P, C.c_double, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "hmsg_test_overlap": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int64, _P, C.c_double, _P, _P, _P]),
    "hmsg_test_pair_overlaps": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int64, _P, C.c_double, _P]),
    "hmsg_test_pool_rows": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64, C.c_int32, C.c_double, C.c_int32, _P]),
    "hmsg_test_graph_early_objects": (C.c_int, [_P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "hmsg_test_sam_post_last": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "hmsg_nav_seeded_fields": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, _P]),
    "hmsg_nav_building_fields": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P, _P, _P]),
    "hmsg_nav_building_paths": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int64,
                                          C.POINTER(C.c_int64)]),
    "hmsg_nav_building_route": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, _P, C.c_int64, _P, _P]),
    "hmsg_test_nav_building_last": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "hmsg_nav_room_labels": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, _P]),
    "hmsg_nav_doors": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P]),
    "hmsg_nav_path_rooms": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64, _P, _P, _P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "hmsg_nav_room_doors": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, _P]),
    "hmsg_test_nav_rooms_last": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "hmsg_test_nav_last": (C.c_int, [C.POINTER(C.c_int32)]),
    "hmsg_test_nav_route_last": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "hmsg_test_knn_last_phase2": (C.c_int64, []),
}
EXPORTED_SYMBOLS = tuple(_SIGS)


class HmsgLib:
    def __init__(self, path: str | None = None):
        path = path or LIB_PATH
        if not os.path.exists(path):
            raise HmsgError(
                f"{path} not found: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()' "
                "or make -C holoagent_amd/csrc).  There is no CPU fallback.")
        self.path = path
        self.c = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(self.c, name)
            fn.restype = res
            fn.argtypes = args
        if self.c.hmsg_config_size() != C.sizeof(HmsgConfig):     # (a stale struct would let hmsg_default_config write past it)
            raise HmsgError("struct hmsg_config of %s has %d bytes, the binding's HmsgConfig %d: rebuild the library or update "
                            "holoagent_amd/_lib.py" % (path, self.c.hmsg_config_size(), C.sizeof(HmsgConfig)))

    def default_config(self, **over) -> HmsgConfig:
        cfg = HmsgConfig()
        self.c.hmsg_default_config(C.byref(cfg))
        for k, v in over.items():
            if not hasattr(cfg, k):
                raise HmsgError(f"unknown config key {k}")
            setattr(cfg, k, v)
        return cfg


_default = None


def lib() -> HmsgLib:
    global _default
    if _default is None:
        _default = HmsgLib()
    return _default


def _ptr(a):
    """numpy array / torch tensor (host or device) / int -> void*"""
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
        return C.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):
        assert a.is_contiguous()
        # A device tensor may still be in the making on torch's current stream (an all-reduce under the nccl backend
        # only makes that stream wait; a dtype conversion is a kernel).  The library works on its own non-blocking
        # stream, which has no ordering against torch's: drain torch's stream before the pointer leaves.  (In the other
        # direction every entry point that writes into a caller's buffer waits for its own stream before returning.)
        if getattr(a, "is_cuda", False):
            import torch
            torch.cuda.current_stream(a.device).synchronize()
        return C.c_void_p(a.data_ptr())
    raise TypeError(type(a))


def lsap(cost, maximize=False, lib_=None):
    """scipy.optimize.linear_sum_assignment(cost, maximize) restated in the library (include/hmsg.h: hmsg_lsap): the same
    (row_ind, col_ind), index for index, also among equally good assignments.  cost: 2-D, numpy or a torch tensor (copied to the host)."""
    L = lib_ or lib()
    if hasattr(cost, "detach"):
        cost = cost.detach().cpu().numpy()
    cost = np.ascontiguousarray(cost, np.float64)
    if cost.ndim != 2:
        raise HmsgError("lsap: expected a matrix (found a %d-D array)" % cost.ndim)
    nr, nc = cost.shape
    n = min(nr, nc)
    row, col = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    got = C.c_int32(0)
    rc = L.c.hmsg_lsap(nr, nc, _ptr(cost), int(bool(maximize)), _ptr(row), _ptr(col), C.byref(got))
    if rc != 0:
        raise HmsgError(f"hmsg_lsap failed ({rc}) (the message is on stderr)")
    return row[:got.value].astype(np.int64), col[:got.value].astype(np.int64)


class EvalCounts(C.Structure):
    """hmsg_eval_counts (include/hmsg.h)"""
    _fields_ = [("tp", C.c_int64), ("tn", C.c_int64), ("fp", C.c_int64), ("fn", C.c_int64), ("acc", C.c_double), ("prec", C.c_double),
                ("recall", C.c_double)]

    def as_dict(self):
        return dict(tp=int(self.tp), tn=int(self.tn), fp=int(self.fp), fn=int(self.fn), acc=float(self.acc), prec=float(self.prec),
                    recall=float(self.recall))


class EvalGt(C.Structure):
    """hmsg_eval_gt (include/hmsg.h)"""
    _fields_ = [("n_floors", C.c_int32), ("floor_lower", _P), ("floor_upper", _P),
                ("n_rooms", C.c_int32), ("room_pts", _P), ("room_off", _P), ("room_min_h", _P), ("room_max_h", _P), ("room_mean_h", _P),
                ("n_objects", C.c_int32), ("obj_pts", _P), ("obj_off", _P), ("obj_obb_center", _P), ("obj_obb_dims", _P), ("obj_name_id", _P),
                ("n_classes", C.c_int32), ("feat_dim", C.c_int32), ("text_feats", _P), ("class_name_id", _P)]


class EvalParams(C.Structure):
    """hmsg_eval_params (include/hmsg.h)"""
    _fields_ = [("eval_metric", C.c_int32), ("room_radius", C.c_double), ("object_radius", C.c_double), ("voxel", C.c_double),
                ("n_top_k", C.c_int32), ("top_k", _P)]


class EvalMetrics(C.Structure):
    """hmsg_eval_metrics (include/hmsg.h)"""
    _fields_ = [("floors", EvalCounts), ("room_acc50", C.c_double), ("room_ap", C.c_double), ("room_prec50", C.c_double),
                ("room_recall50", C.c_double), ("room_gt", C.c_int32), ("room_pred", C.c_int32), ("room_hydra_prec", C.c_double),
                ("room_hydra_recall", C.c_double), ("obj_ap", C.c_double), ("obj_gt", C.c_int32), ("obj_pred", C.c_int32),
                ("obj_iou50", EvalCounts), ("obj_top_k_auc", C.c_double), ("obj_assigned", C.c_int32)]


def _eval_ck(rc, what):
    if rc != 0:
        raise HmsgError(f"{what} failed ({rc}) (the message is on stderr)")


def _pairs32(M, row, col):
    M = np.ascontiguousarray(M, np.float64)
    if M.ndim != 2:
        raise HmsgError("expected a matrix (found a %d-D array)" % M.ndim)
    row, col = np.ascontiguousarray(row, np.int32).reshape(-1), np.ascontiguousarray(col, np.int32).reshape(-1)
    if len(row) != len(col):
        raise HmsgError("row_ind and col_ind differ in length")
    return M, row, col


def eval_floors(gt_lower, gt_upper, pred_vertices, lib_=None):
    """evaluate_floors' counts and ratios (include/hmsg.h: hmsg_eval_floors): gt bounds [Fg] each, predicted floor vertices
    [Fp, 8, 3].  Raises HmsgError on unequal floor counts.  -> dict(tp, tn, fp, fn, acc, prec, recall)"""
    L = lib_ or lib()
    lo, up = np.ascontiguousarray(gt_lower, np.float64).reshape(-1), np.ascontiguousarray(gt_upper, np.float64).reshape(-1)
    v = np.ascontiguousarray(pred_vertices, np.float64).reshape(-1, 8, 3)
    if len(lo) != len(up):
        raise HmsgError("eval_floors: lower and upper bounds differ in length")
    out = EvalCounts()
    _eval_ck(L.c.hmsg_eval_floors(_ptr(lo), _ptr(up), len(lo), _ptr(v), len(v), C.byref(out)), "hmsg_eval_floors")
    return out.as_dict()


def eval_metrics_from_matrix(M, row_ind, col_ind, which_index=6, lib_=None):
    """The threshold sweep of a matrix under an assignment (include/hmsg.h: hmsg_eval_metrics_from_matrix)
    -> (ap, acc, prec, recall) with the last three read at which_index (recall from the sorted list)."""
    L = lib_ or lib()
    M, row, col = _pairs32(M, row_ind, col_ind)
    o = [C.c_double(0) for _ in range(4)]
    _eval_ck(L.c.hmsg_eval_metrics_from_matrix(_ptr(M), M.shape[0], M.shape[1], _ptr(row), _ptr(col), len(row), int(which_index),
                                               *[C.byref(v) for v in o]), "hmsg_eval_metrics_from_matrix")
    return tuple(v.value for v in o)


def eval_counts_at(M, row_ind, col_ind, threshold=0.5, lib_=None):
    """TP / FP / FN and the three ratios at one threshold (include/hmsg.h: hmsg_eval_counts_at)"""
    L = lib_ or lib()
    M, row, col = _pairs32(M, row_ind, col_ind)
    out = EvalCounts()
    _eval_ck(L.c.hmsg_eval_counts_at(_ptr(M), M.shape[0], M.shape[1], _ptr(row), _ptr(col), len(row), float(threshold), C.byref(out)),
             "hmsg_eval_counts_at")
    return out.as_dict()


def eval_hydra_means(over_pred, over_gt, lib_=None):
    """(hydra_prec, hydra_recall) of the two room matrices (include/hmsg.h: hmsg_eval_hydra_means)"""
    L = lib_ or lib()
    a, b = np.ascontiguousarray(over_pred, np.float64), np.ascontiguousarray(over_gt, np.float64)
    if a.ndim != 2 or a.shape != b.shape:
        raise HmsgError("eval_hydra_means: two matrices of one shape expected")
    hp, hr = C.c_double(0), C.c_double(0)
    _eval_ck(L.c.hmsg_eval_hydra_means(_ptr(a), _ptr(b), a.shape[0], a.shape[1], C.byref(hp), C.byref(hr)), "hmsg_eval_hydra_means")
    return hp.value, hr.value


def eval_top_k(rank, n_classes, top_k, lib_=None):
    """({k: accuracy}, top_k_auc) from the ranks of hmsg_eval_semantic_ranks (include/hmsg.h: hmsg_eval_top_k)"""
    L = lib_ or lib()
    rank = np.ascontiguousarray(rank, np.int32).reshape(-1)
    ks = np.ascontiguousarray(list(top_k), np.int32).reshape(-1)
    acc = np.zeros(max(len(ks), 1))
    auc = C.c_double(0)
    _eval_ck(L.c.hmsg_eval_top_k(_ptr(rank), len(rank), int(n_classes), _ptr(ks), len(ks), _ptr(acc), C.byref(auc)), "hmsg_eval_top_k")
    return {int(k): float(a) for k, a in zip(ks, acc)}, auc.value


class SemsegScores(C.Structure):
    """hmsg_semseg_scores (include/hmsg.h)"""
    _fields_ = [("miou", C.c_double), ("fmiou", C.c_double), ("acc", C.c_double), ("macc", C.c_double)]

    def as_dict(self):
        return dict(miou=float(self.miou), fmiou=float(self.fmiou), acc=float(self.acc), macc=float(self.macc))


def semseg_metrics(confusion, ignore=(), lib_=None):
    """metric.py's numbers from a confusion matrix [L, L] (rows ground truth, columns prediction; include/hmsg.h:
    hmsg_semseg_metrics).  `ignore`: class indices in [0, L).  -> dict(miou, fmiou, acc, macc, per_class_iou float64 [L]: NaN for a
    class on neither side, 0 for an ignored one)"""
    L = lib_ or lib()
    conf = np.ascontiguousarray(confusion, np.int64)
    if conf.ndim != 2 or conf.shape[0] != conf.shape[1]:
        raise HmsgError("semseg_metrics: a square matrix expected")
    ig = np.ascontiguousarray(list(ignore), np.int32).reshape(-1)
    out = SemsegScores()
    pc = np.zeros(conf.shape[0], np.float64)
    _eval_ck(L.c.hmsg_semseg_metrics(_ptr(conf), conf.shape[0], _ptr(ig) if len(ig) else None, len(ig), C.byref(out), _ptr(pc)),
             "hmsg_semseg_metrics")
    d = out.as_dict()
    d["per_class_iou"] = pc
    return d


class Comm:
    """RCCL communicator behind the C ABI (include/hmsg.h: hmsg_comm_*).  `Comm.single()` = one rank, no communicator (every
    collective is the identity); `Comm.from_torch(device_id)` = the ranks of an initialised torch.distributed job: rank 0
    makes the id, the process group carries the 128 bytes to the others, every rank joins with its own GPU."""

    def __init__(self, h, rank, world, lib_):
        self.h, self.rank, self.world, self.L = h, rank, world, lib_

    @classmethod
    def single(cls, device_id=0, lib_=None):
        L = lib_ or lib()
        h = _P()
        rc = L.c.hmsg_comm_create(None, 0, 1, int(device_id), C.byref(h))
        if rc != 0:
            raise HmsgError(f"hmsg_comm_create failed ({rc})")
        return cls(h, 0, 1, L)

    @classmethod
    def create(cls, uid: bytes, rank, world, device_id=0, lib_=None):
        L = lib_ or lib()
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(uid))
        h = _P()
        rc = L.c.hmsg_comm_create(C.cast(buf, _P), int(rank), int(world), int(device_id), C.byref(h))
        if rc != 0:
            raise HmsgError(f"hmsg_comm_create failed ({rc}): " + (L.c.hmsg_comm_last_error(None) or b"").decode())
        return cls(h, int(rank), int(world), L)

    @staticmethod
    def unique_id(lib_=None) -> bytes:
        L = lib_ or lib()
        buf = (C.c_uint8 * 128)()
        rc = L.c.hmsg_comm_unique_id(C.cast(buf, _P))
        if rc != 0:
            raise HmsgError(f"hmsg_comm_unique_id failed ({rc}): " + (L.c.hmsg_comm_last_error(None) or b"").decode())
        return bytes(buf)

    @classmethod
    def from_torch(cls, device_id=0, lib_=None, group=None):
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        box = [None]
        if rank == 0:
            try:
                box[0] = cls.unique_id(lib_)
            except HmsgError:
                box[0] = None                    # (told to the others below: every rank takes the same way out)
        dist.broadcast_object_list(box, src=0, group=group)
        if box[0] is None:
            raise HmsgError("hmsg_comm_unique_id failed on rank 0 (librccl could not be loaded)")
        try:
            c = cls.create(box[0], rank, world, device_id, lib_)
        except HmsgError:
            c = None
        oks = [None] * world
        dist.all_gather_object(oks, c is not None, group=group)
        if not all(oks):
            if c is not None:
                c.close()
            raise HmsgError("hmsg_comm_create failed on ranks %s" % [r for r, ok in enumerate(oks) if not ok])
        return c

    def close(self):
        if getattr(self, "h", None):
            self.L.c.hmsg_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scene:
    """One HMSG scene resident on one GPU (thin handle wrapper over the C ABI)."""

    def __init__(self, cfg: HmsgConfig | None = None, lib_: HmsgLib | None = None, **over):
        self.L = lib_ or lib()
        self.cfg = cfg or self.L.default_config(**over)
        h = _P()
        rc = self.L.c.hmsg_create(C.byref(self.cfg), C.byref(h))
        if rc != 0:
            raise HmsgError(f"hmsg_create failed ({rc})")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.c.hmsg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise HmsgError(f"[{rc}] " + self.L.c.hmsg_last_error(self.h).decode())

    @property
    def HW(self):
        return self.cfg.height * self.cfg.width

    def reset(self):
        self._ck(self.L.c.hmsg_reset(self.h))

    def set_profiling(self, on: bool):
        self._ck(self.L.c.hmsg_set_profiling(self.h, int(on)))

    def profile(self):
        """{kernel name: (launches, total_ms, total algorithmic bytes or FLOP)} from the HIP-event brackets
        recorded since the last reset."""
        out = {}
        for i in range(int(self.L.c.hmsg_profile_count(self.h))):
            name = C.create_string_buffer(64)
            n = C.c_int64()
            ms = C.c_double()
            wk = C.c_double()
            self._ck(self.L.c.hmsg_profile_entry(self.h, i, name, C.byref(n), C.byref(ms), C.byref(wk)))
            out[name.value.decode()] = (int(n.value), float(ms.value), float(wk.value))
        return out

    # ---- build
    def add_frames(self, rgb, depth, pose, K):
        n = int(depth.shape[0])
        self._ck(self.L.c.hmsg_add_frames(self.h, n, _ptr(rgb), _ptr(depth), _ptr(pose), _ptr(K)))

    def finalize_map(self):
        self._ck(self.L.c.hmsg_finalize_map(self.h))

    def map_size(self):
        return int(self.L.c.hmsg_map_size(self.h))

    def num_tie_queries(self):
        return int(self.L.c.hmsg_num_tie_queries(self.h))

    def map_size_unfiltered(self):
        return int(self.L.c.hmsg_map_size_unfiltered(self.h))

    def map_points(self, colors=False):
        V = self.map_size()
        xyz = np.empty((V, 3), np.float64)
        rgb = np.empty((V, 3), np.float64) if colors else None
        self._ck(self.L.c.hmsg_get_map_points(self.h, _ptr(xyz), _ptr(rgb)))
        return (xyz, rgb) if colors else xyz

    def add_frame_features(self, first, masks, f_g, f_masked, f_crop, n_masks=None):
        """masks u8 [n, M, H, W], f_g [n, D], f_masked / f_crop [n, M, D]; n_masks i32 [n] = real masks per frame
        (rows beyond it are padding), None = M for all."""
        n, M = int(f_masked.shape[0]), int(f_masked.shape[1])
        nm = None if n_masks is None else np.ascontiguousarray(n_masks, dtype=np.int32)
        self._ck(self.L.c.hmsg_add_frame_features(self.h, first, n, M, _ptr(masks), _ptr(f_g), _ptr(f_masked), _ptr(f_crop),
                                                  _ptr(nm)))

    def add_frame_features_rle(self, first, rles, f_g, f_masked, f_crop):
        """The same hand-over with the masks as SAM's uncompressed run-length records (holoagent_amd/rle.py; include/hmsg.h:
        hmsg_add_frame_features_rle): rles = (counts u32, run_off i64 [T + 1], n_masks i32 [n]) as rle.pack makes them -- numpy
        arrays or torch device tensors -- or a list (frames) of lists (masks) of counts, which is packed here.  f_g [n, D],
        f_masked / f_crop [n, M, D] with M >= every frame's mask count.  No dense mask is built."""
        if isinstance(rles, (list,)) or (isinstance(rles, tuple) and len(rles) != 3):
            from . import rle as _rle
            rles = _rle.pack(rles)
        counts, run_off, n_masks = rles
        if isinstance(counts, np.ndarray) or not hasattr(counts, "data_ptr"):
            counts = np.ascontiguousarray(counts, dtype=np.uint32)
        if isinstance(run_off, np.ndarray) or not hasattr(run_off, "data_ptr"):
            run_off = np.ascontiguousarray(run_off, dtype=np.int64)
        if isinstance(n_masks, np.ndarray) or not hasattr(n_masks, "data_ptr"):
            n_masks = np.ascontiguousarray(n_masks, dtype=np.int32)
        n, M = int(f_masked.shape[0]), int(f_masked.shape[1])
        assert int(n_masks.shape[0]) == n, "n_masks: one entry per frame of f_masked"
        self._ck(self.L.c.hmsg_add_frame_features_rle(self.h, first, n, M, _ptr(counts), _ptr(run_off), _ptr(n_masks), _ptr(f_g),
                                                      _ptr(f_masked), _ptr(f_crop)))

    def frame_num_masks(self, frame):
        return int(self.L.c.hmsg_get_frame_num_masks(self.h, frame))

    def fuse_frames(self):
        self._ck(self.L.c.hmsg_fuse_frames(self.h))

    def map_feats(self, counter=False):
        V, D = self.map_size(), self.cfg.feat_dim
        f = np.empty((V, D), np.float32)
        c = np.empty((V,), np.float32) if counter else None
        self._ck(self.L.c.hmsg_get_map_feats(self.h, _ptr(f), _ptr(c)))
        return (f, c) if counter else f

    def feature_sums(self):
        V, D = self.map_size(), self.cfg.feat_dim
        s_, c = np.empty((V, D), np.float32), np.empty((V,), np.uint32)
        self._ck(self.L.c.hmsg_get_feature_sums(self.h, _ptr(s_), _ptr(c)))
        return s_, c

    def set_feature_sums(self, sums, counter):
        self._ck(self.L.c.hmsg_set_feature_sums(self.h, _ptr(np.ascontiguousarray(sums, np.float32)),
                                                _ptr(np.ascontiguousarray(counter, np.uint32))))

    def frame_nn(self, frame):
        idx = np.empty((self.cfg.height, self.cfg.width), np.int32)
        self._ck(self.L.c.hmsg_get_frame_nn(self.h, frame, _ptr(idx)))
        return idx

    def frame_fp(self, frame):
        out = np.empty((self.frame_num_masks(frame), self.cfg.feat_dim), np.float32)
        self._ck(self.L.c.hmsg_get_frame_fp(self.h, frame, _ptr(out)))
        return out

    def frame_masks3d(self, frame):
        M = self.frame_num_masks(frame)
        sizes = np.empty((M,), np.int64)
        self._ck(self.L.c.hmsg_get_frame_mask_sizes(self.h, frame, _ptr(sizes)))
        pts = np.empty((int(sizes.sum()), 3), np.float64)
        if pts.shape[0]:
            self._ck(self.L.c.hmsg_get_frame_mask_points(self.h, frame, _ptr(pts)))
        off = np.concatenate([[0], np.cumsum(sizes)])
        return [pts[off[i]:off[i + 1]] for i in range(M)]

    def merge_instances(self):
        self._ck(self.L.c.hmsg_merge_instances(self.h))

    def set_frame_window(self, first_frame):
        self._ck(self.L.c.hmsg_set_frame_window(self.h, int(first_frame)))

    def set_merge_tree_batch(self, max_batch_points):
        """How the hierarchical merge walks a level of its tree (include/hmsg.h: hmsg_set_merge_tree_batch): 0 pair by pair (the
        default), n > 0 level batches of at most n input points, -1 a whole level per batch.  Same instances either way."""
        self._ck(self.L.c.hmsg_set_merge_tree_batch(self.h, int(max_batch_points)))

    def merge_tree_local(self, total_frames):
        """-> (threshold of the next level, lists at that level, index of this handle's list)"""
        th, n, i = C.c_double(), C.c_int64(), C.c_int64()
        self._ck(self.L.c.hmsg_merge_tree_local(self.h, int(total_frames), C.byref(th), C.byref(n), C.byref(i)))
        return float(th.value), int(n.value), int(i.value)

    def merge_tree_join(self, clouds, th, final_pass):
        """clouds: list of [n, 3] f64 arrays of the partner handle (may be empty)."""
        sizes = np.array([len(c) for c in clouds], np.int64)
        pts = np.ascontiguousarray(np.concatenate(clouds) if len(clouds) and sizes.sum() else np.zeros((0, 3)), np.float64)
        self._ck(self.L.c.hmsg_merge_tree_join(self.h, len(clouds), _ptr(sizes) if len(clouds) else None,
                                               _ptr(pts) if len(pts) else None, float(th), int(bool(final_pass))))

    def merge_tree_join_raw(self, sizes, points, th, final_pass):
        """Same, the partner's clouds as one block: sizes i64 [n] (host), points [sum, 3] f64 -- a numpy array or a torch
        tensor on the host or ON THE DEVICE (e.g. what an RCCL recv just filled)."""
        sizes = np.ascontiguousarray(sizes, np.int64)
        total = int(sizes.sum())
        self._ck(self.L.c.hmsg_merge_tree_join(self.h, len(sizes), _ptr(sizes) if len(sizes) else None,
                                               _ptr(points) if total else None, float(th), int(bool(final_pass))))

    def instance_sizes(self):
        n = int(self.L.c.hmsg_num_instances(self.h))
        sizes = np.empty((n,), np.int64)
        if n:
            self._ck(self.L.c.hmsg_get_instance_sizes(self.h, _ptr(sizes)))
        return sizes

    def instance_points_into(self, out):
        """Instance points into a caller-supplied [sum, 3] f64 buffer (numpy array, or torch tensor on host or device)."""
        self._ck(self.L.c.hmsg_get_instance_points(self.h, _ptr(out)))

    def feature_sums_into(self, sums, counter):
        """Per-voxel feature sums f32 [V, D] and frame counters u32 [V] into caller-supplied buffers (host or device)."""
        self._ck(self.L.c.hmsg_get_feature_sums(self.h, _ptr(sums), _ptr(counter)))

    def set_feature_sums_from(self, sums, counter):
        """Install feature sums / counters from caller-supplied buffers (host or device) without a detour over numpy."""
        self._ck(self.L.c.hmsg_set_feature_sums(self.h, _ptr(sums), _ptr(counter)))

    def instances(self):
        n = int(self.L.c.hmsg_num_instances(self.h))
        sizes = np.empty((n,), np.int64)
        self._ck(self.L.c.hmsg_get_instance_sizes(self.h, _ptr(sizes)))
        pts = np.empty((int(sizes.sum()), 3), np.float64)
        if pts.shape[0]:
            self._ck(self.L.c.hmsg_get_instance_points(self.h, _ptr(pts)))
        off = np.concatenate([[0], np.cumsum(sizes)])
        return [pts[off[i]:off[i + 1]] for i in range(n)]

    def num_instances(self):
        return int(self.L.c.hmsg_num_instances(self.h))

    def instance_boxes(self):
        n = self.num_instances()
        out = np.empty((n, 6), np.float64)
        if n:
            self._ck(self.L.c.hmsg_get_instance_boxes(self.h, _ptr(out)))
        return out

    def instance_room_share(self, room_vertices, radius=0.2):
        """room_vertices: list of [n_r, 2] (x, z) arrays -> share f64 [N, R] (find_intersection_share on device)."""
        R = len(room_vertices)
        off = np.zeros(R + 1, np.int64)
        off[1:] = np.cumsum([len(v) for v in room_vertices])
        verts = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64).reshape(-1, 2) for v in room_vertices])
                                     if off[-1] else np.zeros((1, 2)), dtype=np.float64)
        out = np.zeros((self.num_instances(), R), np.float64)
        self._ck(self.L.c.hmsg_instance_room_share(self.h, R, _ptr(off), _ptr(verts), float(radius), _ptr(out)))
        return out

    def build_object_nodes(self, floor_zero, floor_height, room_floor, room_vertices, label_feats=None):
        """A10 on the device (segment_hmsg_objects, graph.py:1582-1736, minus the per-view visibility test): returns the
        node records (numpy structured array: instance, floor, room, counter, label, n_points)."""
        nf, R = len(floor_zero), len(room_vertices)
        fz = np.ascontiguousarray(floor_zero, np.float64)
        fh = np.ascontiguousarray(floor_height, np.float64)
        rf = np.ascontiguousarray(room_floor, np.int32)
        off = np.zeros(R + 1, np.int64)
        off[1:] = np.cumsum([len(v) for v in room_vertices])
        verts = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64).reshape(-1, 2) for v in room_vertices])
                                     if off[-1] else np.zeros((1, 2)), dtype=np.float64)
        lf = None if label_feats is None else np.ascontiguousarray(label_feats, np.float32)
        self._ck(self.L.c.hmsg_build_object_nodes(self.h, nf, _ptr(fz), _ptr(fh), R, _ptr(rf), _ptr(off), _ptr(verts),
                                                  0 if lf is None else lf.shape[0], _ptr(lf)))
        return self.nodes()

    def nodes(self, embeddings=False):
        n = int(self.L.c.hmsg_num_nodes(self.h))
        rec = (HmsgNode * max(n, 1))()
        emb = np.empty((n, self.cfg.feat_dim), np.float32) if embeddings else None
        if n:
            self._ck(self.L.c.hmsg_get_nodes(self.h, C.cast(rec, _P), _ptr(emb)))
        out = np.array([(r.instance, r.floor, r.room, r.counter, r.label, r.n_points) for r in rec[:n]],
                       dtype=[("instance", "i4"), ("floor", "i4"), ("room", "i4"), ("counter", "i4"), ("label", "i4"), ("n_points", "i8")])
        return (out, emb) if embeddings else out

    def save_objects(self, directory, records, n_threads=0):
        """Bulk writer of the object level (include/hmsg.h: hmsg_save_objects; Object.save object.py:37-57).  `records`:
        dicts with instance, object_id, room_id, name, view_ids, best_view_id (JSON-encoded here, numbers and clouds by
        the library)."""
        import json
        n = len(records)
        arr = (HmsgObjectRecord * max(n, 1))()
        plain = lambda x: x.item() if isinstance(x, np.generic) else x
        for a, r in zip(arr, records):
            a.instance = int(r["instance"])
            a.file_stem = str(r["object_id"]).encode()
            a.object_id_json = json.dumps(plain(r["object_id"])).encode()
            a.room_id_json = json.dumps(plain(r["room_id"])).encode()
            a.name_json = json.dumps(plain(r["name"])).encode()
            a.view_ids_json = json.dumps([plain(v) for v in r["view_ids"]]).encode()
            a.best_view_id_json = json.dumps(plain(r["best_view_id"])).encode()
        self._ck(self.L.c.hmsg_save_objects(self.h, str(directory).encode(), n, C.cast(arr, _P), int(n_threads)))

    def merge_room_objects(self, clouds, names, overlap_threshold=0.01, radius=0.1):
        """Room.merge_objects (room.py:62-129) for the objects of one room (include/hmsg.h: hmsg_merge_room_objects): `clouds` = the
        objects' point arrays in room.objects order, `names` = their names.  Returns the new room.objects list as groups: [key object,
        objects added to it in the reference's order ...] -- the same-name overlap tests run on the device."""
        n = len(clouds)
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(c) for c in clouds])
        pts = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in clouds]) if off[-1] else np.zeros((1, 3)), np.float64)
        ids = {}
        name_id = np.ascontiguousarray([ids.setdefault(str(v), len(ids)) for v in names], np.int32)
        ng = C.c_int32()
        goff = np.zeros(n + 1, np.int32)
        mem = np.zeros(max(n * (n + 1), 1), np.int32)     # (every object can become a key, and a key's list can hold every other object)
        self._ck(self.L.c.hmsg_merge_room_objects(self.h, n, _ptr(pts), _ptr(off), _ptr(name_id), float(overlap_threshold), float(radius),
                                                  C.byref(ng), _ptr(goff), _ptr(mem), len(mem)))
        return [mem[goff[g]:goff[g + 1]].tolist() for g in range(ng.value)]

    def cloud_set_overlaps(self, ptsA, offA, ptsB, offB, pairs, radius, kd=False):
        """find_overlapping_ratio_faiss's two counts for pairs of clouds from two sets (include/hmsg.h: hmsg_cloud_set_overlaps; kd =
        True: find_intersection_share's float64 comparison, hmsg_cloud_set_overlaps_kd).  pts* float64 [N, 3] and off* int64 [n + 1]
        (CSR), pairs int32 [P, 2] = (a, b): numpy arrays or contiguous torch tensors of those dtypes, on the host or the device.
        Returns uint32 [P, 2] (numpy): points of A[a] with a witness in B[b], points of B[b] with one in A[a]."""
        def arg(a, dt):
            if hasattr(a, "data_ptr"):
                if str(a.dtype).split(".")[-1] != np.dtype(dt).name or not a.is_contiguous():
                    raise HmsgError("cloud_set_overlaps: a torch tensor must be contiguous and of dtype %s" % np.dtype(dt).name)
                return a
            return np.ascontiguousarray(a, dt)
        ptsA, ptsB = arg(ptsA, np.float64), arg(ptsB, np.float64)
        offA, offB, pairs = arg(offA, np.int64), arg(offB, np.int64), arg(pairs, np.int32)
        nA, nB = int(offA.shape[0]) - 1, int(offB.shape[0]) - 1
        P = int(pairs.shape[0]) if len(pairs.shape) == 2 else int(pairs.shape[0]) // 2
        counts = np.zeros((P, 2), np.uint32)
        fn = self.L.c.hmsg_cloud_set_overlaps_kd if kd else self.L.c.hmsg_cloud_set_overlaps
        self._ck(fn(self.h, nA, _ptr(ptsA), _ptr(offA), nB, _ptr(ptsB), _ptr(offB), P, _ptr(pairs), float(radius), _ptr(counts)))
        return counts

    def eval_object_matrices(self, pred_clouds, gt_clouds, gt_obb_center, gt_obb_dims, radius=0.02):
        """The two association matrices of evaluate_objects (include/hmsg.h: hmsg_eval_object_matrices): lists of float64 [n, 3]
        clouds, the ground-truth boxes [G, 3] each.  Returns (iou [P, G], overlap [P, G], number of pairs with iou > 0)."""
        def csr(clouds):
            off = np.zeros(len(clouds) + 1, np.int64)
            off[1:] = np.cumsum([len(c) for c in clouds])
            pts = np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in clouds] + [np.zeros((0, 3))])
            return np.ascontiguousarray(pts), off
        P, G = len(pred_clouds), len(gt_clouds)
        pp, po = csr(pred_clouds)
        gp, go = csr(gt_clouds)
        gc = np.ascontiguousarray(gt_obb_center, np.float64).reshape(G, 3)
        gd = np.ascontiguousarray(gt_obb_dims, np.float64).reshape(G, 3)
        iou, ov = np.zeros((P, G)), np.zeros((P, G))
        n = C.c_int64(0)
        self._ck(self.L.c.hmsg_eval_object_matrices(self.h, P, _ptr(pp), _ptr(po), G, _ptr(gp), _ptr(go), _ptr(gc), _ptr(gd), float(radius),
                                                    _ptr(iou), _ptr(ov), C.byref(n)))
        return iou, ov, int(n.value)

    @staticmethod
    def _eval_arg(a, dt, who):
        """numpy array or contiguous torch tensor (host or device) of dtype dt"""
        if hasattr(a, "data_ptr"):
            if str(a.dtype).split(".")[-1] != np.dtype(dt).name or not a.is_contiguous():
                raise HmsgError("%s: a torch tensor must be contiguous and of dtype %s" % (who, np.dtype(dt).name))
            return a
        return np.ascontiguousarray(a, dt)

    def eval_rooms(self, pred_pts, pred_off, pred_zero_level, pred_height, gt_pts, gt_off, gt_min_h, gt_max_h, gt_mean_h, floor_lower,
                   floor_upper, voxel=0.05, radius=0.05):
        """The three room matrices of evaluate_rooms (include/hmsg.h: hmsg_eval_rooms).  Clouds in CSR form (float64 [N, 3], int64
        [n + 1]), the per-room and per-floor scalars float64: numpy arrays or contiguous torch tensors of those dtypes, on the host or
        the device.  The predicted clouds are only read (the reference flattens them in place).
        Returns (assoc, over_pred, over_gt) float64 [P, G] (numpy) and the number of gated cells."""
        f = lambda a: self._eval_arg(a, np.float64, "eval_rooms")
        i = lambda a: self._eval_arg(a, np.int64, "eval_rooms")
        pp, po, zl, ht, gp, go = f(pred_pts), i(pred_off), f(pred_zero_level), f(pred_height), f(gt_pts), i(gt_off)
        mn, mx, me, lo, up = f(gt_min_h), f(gt_max_h), f(gt_mean_h), f(floor_lower), f(floor_upper)
        P, G, F = int(po.shape[0]) - 1, int(go.shape[0]) - 1, int(lo.shape[0])
        for a, n, what in ((zl, P, "pred_zero_level"), (ht, P, "pred_height"), (mn, G, "gt_min_h"), (mx, G, "gt_max_h"), (me, G, "gt_mean_h"),
                           (up, F, "floor_upper")):
            if int(np.prod(tuple(a.shape))) != n:
                raise HmsgError("eval_rooms: %s has %d entries, expected %d" % (what, int(np.prod(tuple(a.shape))), n))
        out = [np.zeros((max(P, 0), max(G, 0))) for _ in range(3)]
        n = C.c_int64(0)
        self._ck(self.L.c.hmsg_eval_rooms(self.h, P, _ptr(pp), _ptr(po), _ptr(zl), _ptr(ht), G, _ptr(gp), _ptr(go), _ptr(mn), _ptr(mx), _ptr(me),
                                          F, _ptr(lo), _ptr(up), float(voxel), float(radius), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), C.byref(n)))
        return out[0], out[1], out[2], int(n.value)

    def eval_semantic_ranks(self, emb, text, class_name_id, target_name_id):
        """Rank of the ground-truth category among the classes by cosine similarity, per assigned pair (include/hmsg.h:
        hmsg_eval_semantic_ranks).  emb [n, D] float32 or float64, text [C, D] float32, class_name_id int32 [C], target_name_id int32
        [n] (-1: not in the vocabulary): numpy arrays or contiguous torch tensors, host or device.  Returns int32 [n] (numpy)."""
        if hasattr(emb, "data_ptr"):
            f64 = str(emb.dtype).split(".")[-1] == "float64"
            emb = self._eval_arg(emb, np.float64 if f64 else np.float32, "eval_semantic_ranks")
        else:
            f64 = np.asarray(emb).dtype == np.float64
            emb = np.ascontiguousarray(emb, np.float64 if f64 else np.float32)
        text = self._eval_arg(text, np.float32, "eval_semantic_ranks")
        cn = self._eval_arg(class_name_id, np.int32, "eval_semantic_ranks")
        tg = self._eval_arg(target_name_id, np.int32, "eval_semantic_ranks")
        if len(emb.shape) != 2 or len(text.shape) != 2 or emb.shape[1] != text.shape[1]:
            raise HmsgError("eval_semantic_ranks: emb [n, D] and text [C, D] expected")
        n, D, Cn = int(emb.shape[0]), int(emb.shape[1]), int(text.shape[0])
        if int(cn.shape[0]) != Cn or int(tg.shape[0]) != n:
            raise HmsgError("eval_semantic_ranks: class_name_id / target_name_id do not fit the tables")
        rank = np.zeros(max(n, 1), np.int32)
        self._ck(self.L.c.hmsg_eval_semantic_ranks(self.h, n, _ptr(emb), int(f64), D, Cn, _ptr(text), _ptr(cn), _ptr(tg), _ptr(rank)))
        return rank[:n]

    def semseg_instance_labels(self, emb, text, class_label):
        """text_prompt + sim_2_label (include/hmsg.h: hmsg_semseg_instance_labels): the class label of the text row with the largest
        float32 cosine, the smaller index among equal ones; a zero embedding gets class_label[0].  emb [n, D] float32 or float64, text
        [C, D] float32, class_label int32 [C]: numpy arrays or contiguous torch tensors, host or device.  Returns int32 [n] (numpy)."""
        if hasattr(emb, "data_ptr"):
            f64 = str(emb.dtype).split(".")[-1] == "float64"
            emb = self._eval_arg(emb, np.float64 if f64 else np.float32, "semseg_instance_labels")
        else:
            f64 = np.asarray(emb).dtype == np.float64
            emb = np.ascontiguousarray(emb, np.float64 if f64 else np.float32)
        text = self._eval_arg(text, np.float32, "semseg_instance_labels")
        cl = self._eval_arg(class_label, np.int32, "semseg_instance_labels")
        if len(emb.shape) != 2 or len(text.shape) != 2 or emb.shape[1] != text.shape[1] or int(cl.shape[0]) != int(text.shape[0]):
            raise HmsgError("semseg_instance_labels: emb [n, D], text [C, D] and class_label [C] expected")
        n = int(emb.shape[0])
        out = np.zeros(max(n, 1), np.int32)
        self._ck(self.L.c.hmsg_semseg_instance_labels(self.h, n, _ptr(emb), int(f64), int(emb.shape[1]), int(text.shape[0]), _ptr(text), _ptr(cl),
                                                      _ptr(out)))
        return out[:n]

    def knn_labels(self, points, labels, queries, k, return_index=False, out=None, out_index=None):
        """knn_interpolation's label transfer (include/hmsg.h: hmsg_knn_labels): points float64 [n, 3] with labels int32 [n] (-1: the
        row is dropped), queries float64 [m, 3], 1 <= k <= 16: numpy arrays or contiguous torch tensors, host or device.  Returns int32
        [m] (with return_index also int32 [m, k]: the neighbours' positions after the drop, in (d2, index) order), as numpy arrays -- or
        written into `out` / `out_index` when given (numpy or torch, host or device), which are then what is returned."""
        pts = self._eval_arg(points, np.float64, "knn_labels")
        lab = self._eval_arg(labels, np.int32, "knn_labels")
        q = self._eval_arg(queries, np.float64, "knn_labels")
        n = int(np.prod(tuple(pts.shape))) // 3
        m = int(np.prod(tuple(q.shape))) // 3
        if int(np.prod(tuple(lab.shape))) != n:
            raise HmsgError("knn_labels: %d points and %d labels" % (n, int(np.prod(tuple(lab.shape)))))
        k = int(k)
        if out is None:
            out = np.zeros(m, np.int32)
        if return_index and out_index is None:
            out_index = np.zeros((m, max(k, 1)), np.int32)
        self._ck(self.L.c.hmsg_knn_labels(self.h, n, _ptr(pts), _ptr(lab), m, _ptr(q), k, _ptr(out), _ptr(out_index) if return_index else None))
        return (out, out_index) if return_index else out

    def knn_last_phase2(self):
        """queries the last knn_labels / evaluate_semseg call finished by scan (include/hmsg_test.h: hmsg_test_knn_last_phase2)"""
        return int(self.L.c.hmsg_test_knn_last_phase2())

    def semseg_confusion(self, gt_label, pred_label, n_labels):
        """confusion matrix int64 [L, L] (rows ground truth, columns prediction) of labels in [0, L) (include/hmsg.h:
        hmsg_semseg_confusion): int32 arrays of one length, numpy or contiguous torch tensors, host or device."""
        g = self._eval_arg(gt_label, np.int32, "semseg_confusion")
        p = self._eval_arg(pred_label, np.int32, "semseg_confusion")
        m = int(np.prod(tuple(g.shape)))
        if int(np.prod(tuple(p.shape))) != m:
            raise HmsgError("semseg_confusion: the label arrays differ in length")
        L_ = int(n_labels)
        conf = np.zeros((max(L_, 1), max(L_, 1)), np.int64)
        self._ck(self.L.c.hmsg_semseg_confusion(self.h, m, _ptr(g), _ptr(p), L_, _ptr(conf)))
        return conf

    def evaluate_semseg(self, text, class_ids, gt_points, gt_labels, k=5, ignore=()):
        """The semantic segmentation score of the pooled scene (include/hmsg.h: hmsg_evaluate_semseg): text float32 [C, D] with the
        class id of every row, ground-truth points float64 [m, 3] with their class ids; ids are arbitrary integers, mapped to [0, L)
        through np.unique of all of them (class_ids and gt_labels on the host).  -> dict(miou, fmiou, acc, macc, per_class_iou {id:
        iou}, confusion int64 [L, L], classes int64 [L])"""
        cid = np.asarray(class_ids).reshape(-1).astype(np.int64)
        gl = np.asarray(gt_labels.detach().cpu().numpy() if hasattr(gt_labels, "detach") else gt_labels).reshape(-1).astype(np.int64)
        classes = np.unique(np.concatenate([cid, gl, np.asarray(list(ignore), np.int64)]))
        L_ = len(classes)
        text = self._eval_arg(text, np.float32, "evaluate_semseg")
        gp = self._eval_arg(gt_points, np.float64, "evaluate_semseg")
        cl = np.ascontiguousarray(np.searchsorted(classes, cid), np.int32)
        g32 = np.ascontiguousarray(np.searchsorted(classes, gl), np.int32)
        ig = np.ascontiguousarray(np.searchsorted(classes, np.asarray(list(ignore), np.int64)), np.int32)
        if len(text.shape) != 2 or int(text.shape[0]) != len(cl):
            raise HmsgError("evaluate_semseg: text [C, D] and C class ids expected")
        m = int(np.prod(tuple(gp.shape))) // 3
        if m != len(g32):
            raise HmsgError("evaluate_semseg: %d ground-truth points and %d labels" % (m, len(g32)))
        sc = SemsegScores()
        pc = np.zeros(L_, np.float64)
        conf = np.zeros((L_, L_), np.int64)
        self._ck(self.L.c.hmsg_evaluate_semseg(self.h, _ptr(text), len(cl), _ptr(cl), _ptr(gp), _ptr(g32), m, int(k), L_,
                                               _ptr(ig) if len(ig) else None, len(ig), C.byref(sc), _ptr(pc), _ptr(conf)))
        d = sc.as_dict()
        d.update(per_class_iou={int(c): float(v) for c, v in zip(classes, pc)}, confusion=conf, classes=classes)
        return d

    def room_clouds(self, y_lo, y_hi, T, z_levels, room_xz):
        """segment_hmsg_room's room clouds on the device (include/hmsg.h: hmsg_room_clouds): room_xz = list of [n, 2] arrays;
        returns (per room the ascending indices into the floor cloud, size of the floor cloud)."""
        T = np.ascontiguousarray(T, np.float64).reshape(16)
        z = np.ascontiguousarray(z_levels, np.float64).reshape(-1)
        off = np.zeros(len(room_xz) + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in room_xz])
        xz = np.ascontiguousarray(np.concatenate([np.asarray(r, np.float64).reshape(-1, 2) for r in room_xz]) if off[-1] else np.zeros((0, 2)))
        sizes = np.zeros(len(room_xz), np.int64)
        nf = C.c_int64(0)
        cap = int(len(room_xz)) * max(int(self.map_size()), 1)
        out = np.empty(cap, np.int32)
        self._ck(self.L.c.hmsg_room_clouds(self.h, float(y_lo), float(y_hi), _ptr(T), len(z), _ptr(z), len(room_xz), _ptr(off), _ptr(xz),
                                           _ptr(sizes), _ptr(out), cap, C.byref(nf)))
        o = np.concatenate([[0], np.cumsum(sizes)])
        self._room_clouds_n = len(room_xz)
        return [out[o[r]:o[r + 1]].copy() for r in range(len(room_xz))], int(nf.value)

    def room_camera_distances(self, cam_xz):
        """camera (x, z) -> distance to every room cloud of the last room_clouds call, on the device (include/hmsg.h:
        hmsg_room_camera_distances); [n, R] f64."""
        q = np.ascontiguousarray(cam_xz, np.float64).reshape(-1, 2)
        out = np.empty((len(q), max(self._room_clouds_n, 1)), np.float64)
        self._ck(self.L.c.hmsg_room_camera_distances(self.h, int(self._room_clouds_n), len(q), _ptr(q), _ptr(out)))
        return out[:, : self._room_clouds_n]

    def object_views(self, poses_inv, wh, K, pair_inst, pair_view, min_visible_ratio=0.5, max_depth=10.0):
        """check_object_in_view (utils/graph_utils.py:95-157) for (instance, view) pairs on the device (include/hmsg.h:
        hmsg_object_views): poses_inv [V, 4, 4] world -> camera, wh [V, 2] image width / height, K [3, 3];
        returns (visible bool [P], mean_depth f64 [P])."""
        P_ = np.ascontiguousarray(poses_inv, np.float64).reshape(-1, 16)
        wh = np.ascontiguousarray(wh, np.int32).reshape(-1, 2)
        assert len(wh) == len(P_)
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        pi = np.ascontiguousarray(pair_inst, np.int32).reshape(-1)
        pv = np.ascontiguousarray(pair_view, np.int32).reshape(-1)
        assert len(pi) == len(pv)
        vis = np.zeros(max(len(pi), 1), np.uint8)
        md = np.full(max(len(pi), 1), np.inf)
        self._ck(self.L.c.hmsg_object_views(self.h, len(P_), _ptr(P_), _ptr(wh), _ptr(K), len(pi), _ptr(pi), _ptr(pv),
                                            float(min_visible_ratio), float(max_depth), _ptr(vis), _ptr(md)))
        return vis[:len(pi)].astype(bool), md[:len(pi)]

    def nav_grid(self, y_lo, y_hi, cell_size=0.03):
        """bounds and grid of the slab y_lo <= y <= y_hi of the map (include/hmsg.h: hmsg_map_nav_grid) -> (pcd_min, pcd_max, (columns, rows))"""
        mn, mx, grid = np.zeros(3), np.zeros(3), np.zeros(2, np.int32)
        self._ck(self.L.c.hmsg_map_nav_grid(self.h, float(y_lo), float(y_hi), float(cell_size), _ptr(mn), _ptr(mx), _ptr(grid)))
        return mn, mx, (int(grid[0]), int(grid[1]))

    def nav_floor_maps(self, y_lo, y_hi, zero_level, poses, params=None, top_down=True, **over):
        """The navigation maps of a slab of the map (include/hmsg.h: hmsg_map_nav_floor_maps): the slab is selected on the device, no
        point of it goes to the host.  y_lo, y_hi, zero_level: a storey of segment_floors().  -> the dict of nav_floor_maps."""
        prm = params if params is not None else nav_params(self.L, **over)
        _, _, (W, H) = self.nav_grid(y_lo, y_hi, prm.cell_size)
        P_ = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
        return _nav_call(H, W, top_down, lambda out: self._ck(
            self.L.c.hmsg_map_nav_floor_maps(self.h, float(y_lo), float(y_hi), float(zero_level), C.byref(prm), len(P_),
                                             _ptr(P_) if len(P_) else None, C.byref(out))))

    def nav_height_map(self, y_lo, y_hi, zero_level, params=None, **over):
        """The height map of a slab of the map (include/hmsg.h, N10: hmsg_map_nav_height_map), selected on the device -> the dict
        of nav_height_map."""
        prm = params if params is not None else height_params(self.L, **over)
        _, _, (W, H) = self.nav_grid(y_lo, y_hi, prm.cell_size)
        return _height_call(H, W, None, lambda top, known, mn, mx, grid: self._ck(
            self.L.c.hmsg_map_nav_height_map(self.h, float(y_lo), float(y_hi), float(zero_level), C.byref(prm), top, known, mn, mx, grid)))

    def segment_floors(self):
        """A8 behind the C ABI (include/hmsg.h: hmsg_segment_floors) -> list of dicts (y_lo, y_hi, zero_level, height,
        bbox_min, bbox_max, n_points)."""
        n = C.c_int32(0)
        self._ck(self.L.c.hmsg_segment_floors(self.h, None, 0, C.byref(n)))
        rec = np.zeros((max(n.value, 1), 11), np.float64)          # hmsg_floor: 10 doubles + one int64
        self._ck(self.L.c.hmsg_segment_floors(self.h, _ptr(rec), n.value, C.byref(n)))
        return [dict(y_lo=r[0], y_hi=r[1], zero_level=r[2], height=r[3], bbox_min=r[4:7].copy(), bbox_max=r[7:10].copy(),
                     n_points=int(r[10:11].view(np.int64)[0])) for r in rec[:n.value]]

    def segment_rooms(self, y_lo, y_hi, zero_level, height, resolution):
        """N1 on the device (include/hmsg.h: hmsg_segment_rooms) -> (markers i32 [rows, cols], n_rooms, xz_min [2])."""
        rows, cols, nr = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        xz = np.zeros(2, np.float64)
        a = (self.h, float(y_lo), float(y_hi), float(zero_level), float(height), float(resolution))
        self._ck(self.L.c.hmsg_segment_rooms(*a, None, 0, C.byref(rows), C.byref(cols), C.byref(nr), _ptr(xz)))
        m = np.empty((rows.value, cols.value), np.int32)
        self._ck(self.L.c.hmsg_segment_rooms(*a, _ptr(m), m.size, C.byref(rows), C.byref(cols), C.byref(nr), _ptr(xz)))
        return m, int(nr.value), xz

    def allgather_nodes(self, comm: "Comm", n_rooms_local: int):
        """Cross-scene retrieval (include/hmsg.h: hmsg_allgather_nodes): the ranks' node tables all-gathered over RCCL, HBM
        to HBM, into one resident index -> (NodeIndex over the global table, node_off [world + 1], room_off [world + 1])."""
        ix = _P()
        node_off = np.zeros(comm.world + 1, np.int64)
        room_off = np.zeros(comm.world + 1, np.int64)
        self._ck(self.L.c.hmsg_allgather_nodes(self.h, comm.h, int(n_rooms_local), C.byref(ix), _ptr(node_off), _ptr(room_off)))
        return NodeIndex._wrap(self.L, ix, int(node_off[-1]), self.cfg.feat_dim), node_off, room_off

    def allreduce_feature_sums(self, comm: "Comm"):
        """One episode fused in disjoint frame windows (include/hmsg.h: hmsg_allreduce_feature_sums): sums and counters of all
        ranks all-reduced in place over RCCL."""
        self._ck(self.L.c.hmsg_allreduce_feature_sums(self.h, comm.h))

    def merge_tree_sharded(self, comm: "Comm", total_frames: int) -> bool:
        """hierarchical_merge of one episode sharded over the ranks, behind the C ABI (include/hmsg.h: hmsg_merge_tree_sharded): local
        levels, agreement, cross-rank joins over ncclSend / ncclRecv.  True on the rank that holds the episode's instances."""
        holds = C.c_int32()
        self._ck(self.L.c.hmsg_merge_tree_sharded(self.h, comm.h, int(total_frames), C.byref(holds)))
        return bool(holds.value)

    def comm_send(self, comm: "Comm", dev_tensor, dst: int):
        self._ck(self.L.c.hmsg_comm_send(self.h, comm.h, _ptr(dev_tensor), int(dev_tensor.numel() * dev_tensor.element_size()), int(dst)))

    def comm_recv(self, comm: "Comm", dev_tensor, src: int):
        self._ck(self.L.c.hmsg_comm_recv(self.h, comm.h, _ptr(dev_tensor), int(dev_tensor.numel() * dev_tensor.element_size()), int(src)))

    def index_from_nodes(self):
        """Resident retrieval index over the node table, gathered on the device."""
        ix = _P()
        self._ck(self.L.c.hmsg_index_from_nodes(self.h, C.byref(ix)))
        return NodeIndex._wrap(self.L, ix, int(self.L.c.hmsg_num_nodes(self.h)), self.cfg.feat_dim)

    def voxel_down_sample(self, points, voxel_size):
        """Open3D voxel_down_sample of an [n, 3] f64 cloud (canonical ascending voxel order) on the device."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        out = np.empty_like(pts)
        n_out = C.c_int64(0)
        self._ck(self.L.c.hmsg_voxel_down_sample(self.h, _ptr(pts), pts.shape[0], float(voxel_size), _ptr(out), C.byref(n_out)))
        return out[: n_out.value].copy()

    def denoise_instances(self, eps=0.05, min_points=10):
        self._ck(self.L.c.hmsg_denoise_instances(self.h, float(eps), int(min_points)))

    def pool_instances(self):
        self._ck(self.L.c.hmsg_pool_instances(self.h))

    def instance_feats(self):
        n = int(self.L.c.hmsg_num_instances(self.h))
        out = np.empty((n, self.cfg.feat_dim), np.float32)
        if n:
            self._ck(self.L.c.hmsg_get_instance_feats(self.h, _ptr(out)))
        return out

    def restore_stage(self, map_points, inst_points, inst_feats, K, map_colors=None, map_feats=None):
        """The stage artefacts back into a fresh (or reset) scene (include/hmsg.h: hmsg_restore_stage): afterwards the scene is where
        pool_instances() leaves one, as far as the graph level can tell.  map_points [V, 3] f64 (any cloud, its order is kept);
        inst_points: a list of [n_i, 3] arrays, or (off i64 [N + 1], xyz [sum, 3] f64) with xyz on the host or the device;
        inst_feats [N, D] f32; K [3, 3]; map_colors [V, 3] f64 and map_feats [V, D] f32 optional.  numpy arrays, or torch tensors
        (host or device) of exactly these dtypes."""
        def arr(a, dt):
            return np.ascontiguousarray(a, dt) if isinstance(a, (np.ndarray, list, tuple)) else a
        if isinstance(inst_points, tuple) and len(inst_points) == 2 and np.ndim(inst_points[0]) == 1:
            off, xyz = np.ascontiguousarray(inst_points[0], np.int64), arr(inst_points[1], np.float64)
        else:
            clouds = [np.asarray(c, np.float64).reshape(-1, 3) for c in inst_points]
            off = np.zeros(len(clouds) + 1, np.int64)
            off[1:] = np.cumsum([len(c) for c in clouds])
            xyz = np.ascontiguousarray(np.concatenate(clouds) if len(clouds) else np.zeros((0, 3)), np.float64)
        n = len(off) - 1
        mp, mc, mf = arr(map_points, np.float64), None if map_colors is None else arr(map_colors, np.float64), None if map_feats is None else arr(map_feats, np.float32)
        feats = arr(inst_feats, np.float32)
        D = self.cfg.feat_dim
        if tuple(feats.shape) != (n, D) and not (n == 0 and int(np.prod(tuple(feats.shape))) == 0):
            raise ValueError(f"inst_feats must be [{n}, {D}], got {tuple(feats.shape)}")
        if mf is not None and tuple(mf.shape) != (int(mp.shape[0]), D):
            raise ValueError(f"map_feats must be [{int(mp.shape[0])}, {D}], got {tuple(mf.shape)}")
        if mc is not None and tuple(mc.shape) != tuple(mp.shape):
            raise ValueError("map_colors must have the shape of map_points")
        Kh = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
        self._ck(self.L.c.hmsg_restore_stage(self.h, int(mp.shape[0]), _ptr(mp), _ptr(mc), _ptr(mf), n, _ptr(off),
                                             _ptr(xyz) if int(off[-1]) else None, _ptr(feats) if n else None, _ptr(Kh)))


def read_ply(path, lib_: "HmsgLib | None" = None):
    """x y z of a binary little-endian PLY file as f64 [n, 3] (include/hmsg.h: hmsg_read_ply)."""
    L = lib_ or lib()
    n = C.c_int64(0)
    rc = L.c.hmsg_read_ply(str(path).encode(), None, 0, C.byref(n))
    if rc != 0:
        raise HmsgError(f"hmsg_read_ply failed ({rc}) for {path}")
    out = np.empty((int(n.value), 3), np.float64)
    rc = L.c.hmsg_read_ply(str(path).encode(), _ptr(out), int(n.value), C.byref(n))
    if rc != 0:
        raise HmsgError(f"hmsg_read_ply failed ({rc}) for {path}")
    return out


class SceneGraph:
    """The graph as one object behind the C ABI (include/hmsg.h: hmsg_build_graph / hmsg_graph_begin + _finish, hmsg_save, hmsg_load,
    hmsg_graph_query) -- floors -> rooms -> views -> objects -> edges held by the library."""

    def __init__(self, L, g, D, scene=None):
        self.L, self.g, self.D, self.scene = L, g, int(D), scene
        self._keep = []

    @staticmethod
    def _params(L, **over):
        p = HmsgGraphParams()
        L.c.hmsg_graph_default_params(C.byref(p))
        for k, v in over.items():
            setattr(p, k, v)
        return p

    @staticmethod
    def _strs(items):
        if items is None:
            return None, None
        enc = [None if s is None else str(s).encode() for s in items]
        arr = (C.c_char_p * max(len(enc), 1))(*enc)
        return arr, enc

    @classmethod
    def begin(cls, scene: "Scene", poses, view_feats, poses_inv=None, img_paths=None, **params):
        """the room level right after hmsg_finalize_map (device stage now, KMeans on host threads -- kmeans_device=1: in one batched
        call per storey on the device); finish() after the pooling"""
        L = scene.L
        P_ = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
        Pi = None if poses_inv is None else np.ascontiguousarray(np.asarray(poses_inv, np.float64).reshape(-1, 16))
        Fg = np.ascontiguousarray(np.asarray(view_feats, np.float32).reshape(len(P_), -1))
        assert Fg.shape[1] == scene.cfg.feat_dim and (Pi is None or Pi.shape == P_.shape)
        paths, keep = cls._strs(img_paths)
        prm = cls._params(L, **params)
        g = _P()
        scene._ck(L.c.hmsg_graph_begin(scene.h, C.byref(prm), len(P_), _ptr(P_), None if Pi is None else _ptr(Pi), _ptr(Fg),
                                       None if paths is None else C.cast(paths, _P), C.byref(g)))
        return cls(L, g, scene.cfg.feat_dim, scene)

    def finish(self, label_feats=None, label_names=None):
        lf = None if label_feats is None else np.ascontiguousarray(np.asarray(label_feats, np.float32))
        names, keep = self._strs(label_names if lf is not None else None)
        self._ck(self.L.c.hmsg_graph_finish(self.g, 0 if lf is None else len(lf), None if lf is None else _ptr(lf),
                                            None if names is None else C.cast(names, _P)))
        return self

    @classmethod
    def build(cls, scene, poses, view_feats, label_feats=None, label_names=None, poses_inv=None, img_paths=None, **params):
        return cls.begin(scene, poses, view_feats, poses_inv=poses_inv, img_paths=img_paths, **params).finish(label_feats, label_names)

    @classmethod
    def load(cls, directory, device_id=0, lib_: "HmsgLib | None" = None):
        L = lib_ or lib()
        g = _P()
        rc = L.c.hmsg_load(str(directory).encode(), int(device_id), C.byref(g))
        if rc != 0:
            raise HmsgError(f"hmsg_load failed ({rc}) for {directory}")
        return cls(L, g, 0)

    def _ck(self, rc):
        if rc != 0:
            raise HmsgError(self.L.c.hmsg_graph_last_error(self.g).decode() + f" (rc={rc})")

    def close(self):
        if self.g:
            self.L.c.hmsg_graph_destroy(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def counts(self):
        c = HmsgGraphCounts()
        self._ck(self.L.c.hmsg_graph_get_counts(self.g, C.byref(c)))
        return {k: getattr(c, k) for k, _ in HmsgGraphCounts._fields_}

    def edges(self):
        n = C.c_int64(0)
        self._ck(self.L.c.hmsg_graph_get_edges(self.g, None, 0, C.byref(n)))
        e = np.zeros((max(n.value, 1), 2), np.int64)
        self._ck(self.L.c.hmsg_graph_get_edges(self.g, _ptr(e), n.value, C.byref(n)))
        return e[: n.value]

    def objects(self):
        n = self.counts()["objects"]
        arr = (HmsgGraphObject * max(n, 1))()
        self._ck(self.L.c.hmsg_graph_get_objects(self.g, C.cast(arr, _P), n))
        return [dict(object_id=a.object_id.decode(), name=a.name.decode(), room=a.room, instance=a.instance, label=a.label,
                     n_views=a.n_views, best_view=a.best_view) for a in arr[:n]]

    def rooms(self):
        n = self.counts()["rooms"]
        arr = (HmsgGraphRoom * max(n, 1))()
        self._ck(self.L.c.hmsg_graph_get_rooms(self.g, C.cast(arr, _P), n))
        return [dict(room_id=a.room_id.decode(), name=a.name.decode(), floor=a.floor, n_vertices=a.n_vertices, n_points=a.n_points,
                     n_embeddings=a.n_embeddings, n_sample_images=a.n_sample_images, n_objects=a.n_objects, n_views=a.n_views)
                for a in arr[:n]]

    def room_vertices(self, room, n=None):
        n = int(n if n is not None else self.rooms()[room]["n_vertices"])
        out = np.zeros((max(n, 1), 2), np.float64)
        self._ck(self.L.c.hmsg_graph_get_room_vertices(self.g, int(room), _ptr(out), out.size))
        return out[:n]

    def room_embeddings(self, room, D=None):
        r = self.rooms()[room]
        D = int(D or self.D)
        out = np.zeros((max(r["n_embeddings"], 1), D), np.float32)
        self._ck(self.L.c.hmsg_graph_get_room_embeddings(self.g, int(room), _ptr(out), out.size))
        return out[: r["n_embeddings"]]

    def to_dict(self):
        import json
        n = C.c_int64(0)
        self._ck(self.L.c.hmsg_graph_to_json(self.g, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        self._ck(self.L.c.hmsg_graph_to_json(self.g, buf, n.value, C.byref(n)))
        return json.loads(buf.value.decode())

    def evaluate(self, gt, eval_metric="overlap", top_k=(), room_radius=0.05, object_radius=0.02, voxel=0.05):
        """The reference's evaluate_floors / _rooms / _objects of this graph in one call (include/hmsg.h: hmsg_graph_evaluate).  gt: a
        dict of arrays -- floor_lower, floor_upper; room_clouds (list of [n, 3]), room_min_h, room_max_h, room_mean_h; obj_clouds,
        obj_obb_center, obj_obb_dims, obj_name_id; text_feats [C, D] float32, class_name_id.  Returns the reference's three
        dictionaries' keys: dict(floors=..., rooms=..., objects=dict(instances, instances_iou50, ins_semantics))."""
        def csr(clouds):
            off = np.zeros(len(clouds) + 1, np.int64)
            off[1:] = np.cumsum([len(c) for c in clouds])
            pts = np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in clouds] + [np.zeros((0, 3))])
            return np.ascontiguousarray(pts), off
        f64 = lambda k: np.ascontiguousarray(gt[k], np.float64)
        i32 = lambda k: np.ascontiguousarray(gt[k], np.int32)
        rp, ro = csr(gt["room_clouds"])
        op, oo = csr(gt["obj_clouds"])
        text = np.ascontiguousarray(gt["text_feats"], np.float32)
        keep = dict(lo=f64("floor_lower"), up=f64("floor_upper"), mn=f64("room_min_h"), mx=f64("room_max_h"), me=f64("room_mean_h"),
                    oc=f64("obj_obb_center"), od=f64("obj_obb_dims"), on=i32("obj_name_id"), cn=i32("class_name_id"))
        g = EvalGt(len(keep["lo"]), _ptr(keep["lo"]), _ptr(keep["up"]), len(ro) - 1, _ptr(rp), _ptr(ro), _ptr(keep["mn"]), _ptr(keep["mx"]),
                   _ptr(keep["me"]), len(oo) - 1, _ptr(op), _ptr(oo), _ptr(keep["oc"]), _ptr(keep["od"]), _ptr(keep["on"]), text.shape[0],
                   text.shape[1], _ptr(text), _ptr(keep["cn"]))
        ks = np.ascontiguousarray(list(top_k), np.int32)
        prm = EvalParams()
        self.L.c.hmsg_eval_default_params(C.byref(prm))
        prm.eval_metric = {"iou": 0, "overlap": 1}[eval_metric]
        prm.room_radius, prm.object_radius, prm.voxel = float(room_radius), float(object_radius), float(voxel)
        prm.n_top_k, prm.top_k = len(ks), _ptr(ks) if len(ks) else None
        acc = np.zeros(max(len(ks), 1))
        m = EvalMetrics()
        self._ck(self.L.c.hmsg_graph_evaluate(self.g, C.byref(g), C.byref(prm), C.byref(m), _ptr(acc)))
        fl = m.floors.as_dict()
        i50 = m.obj_iou50.as_dict()
        return dict(
            floors=dict(tp=fl["tp"], tn=fl["tn"], fp=fl["fp"], fn=fl["fn"], acc=fl["acc"], prec=fl["prec"], recall=fl["recall"]),
            rooms={"acc@IoU=0.5": m.room_acc50, "ap": m.room_ap, "prec@IoU=0.5": m.room_prec50, "recall@IoU=0.5": m.room_recall50,
                   "gt": int(m.room_gt), "pred": int(m.room_pred), "hydra_prec": m.room_hydra_prec, "hydra_recall": m.room_hydra_recall},
            objects=dict(instances=dict(ap=m.obj_ap, gt=int(m.obj_gt), pred=int(m.obj_pred)),
                         instances_iou50=dict(acc=i50["acc"], prec=i50["prec"], recall=i50["recall"], tp=i50["tp"], fp=i50["fp"], fn=i50["fn"],
                                              gt=int(m.obj_gt), pred=int(m.obj_pred)),
                         ins_semantics=dict(tp_top_k_acc={int(k): float(a) for k, a in zip(ks, acc)}, top_k_auc=m.obj_top_k_auc)))

    def save(self, directory):
        self._ck(self.L.c.hmsg_save(self.g, str(directory).encode()))

    def nav_grid(self, floor, cell_size=0.03):
        """bounds and grid of a storey's cloud (include/hmsg.h: hmsg_graph_nav_grid) -> (pcd_min [3], pcd_max [3], (columns, rows))"""
        mn, mx, grid = np.zeros(3), np.zeros(3), np.zeros(2, np.int32)
        self._ck(self.L.c.hmsg_graph_nav_grid(self.g, int(floor), float(cell_size), _ptr(mn), _ptr(mx), _ptr(grid)))
        return mn, mx, (int(grid[0]), int(grid[1]))

    def nav_floor_maps(self, floor, poses, params=None, top_down=True, **over):
        """The navigation maps of storey `floor` (include/hmsg.h: hmsg_graph_nav_floor_maps): the map's slab is selected on the
        device, no point of it goes to the host.  poses: [n, 4, 4] camera-to-world.  -> the dict of nav_floor_maps."""
        prm = params if params is not None else nav_params(self.L, **over)
        _, _, (W, H) = self.nav_grid(floor, prm.cell_size)
        P_ = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
        return _nav_call(H, W, top_down, lambda out: self._ck(
            self.L.c.hmsg_graph_nav_floor_maps(self.g, int(floor), C.byref(prm), len(P_), _ptr(P_) if len(P_) else None, C.byref(out))))

    def nav_height_map(self, floor, params=None, **over):
        """The height map of storey `floor` (include/hmsg.h, N10: hmsg_graph_nav_height_map), zero_level the floor's own -> the dict
        of nav_height_map."""
        prm = params if params is not None else height_params(self.L, **over)
        _, _, (W, H) = self.nav_grid(floor, prm.cell_size)
        return _height_call(H, W, None, lambda top, known, mn, mx, grid: self._ck(
            self.L.c.hmsg_graph_nav_height_map(self.g, int(floor), C.byref(prm), top, known, mn, mx, grid)))

    def index(self, room_name_emb=None):
        ix = _P()
        rn = None if room_name_emb is None else np.ascontiguousarray(np.asarray(room_name_emb, np.float64))
        self._ck(self.L.c.hmsg_graph_index(self.g, None if rn is None else _ptr(rn), C.byref(ix)))
        c = self.counts()
        nx = NodeIndex._wrap(self.L, ix, c["objects"], rn.shape[1] if rn is not None else self.D)
        nx._n_rooms = c["rooms"]
        return nx

    def allgather_index(self, comm: "Comm", room_name_emb=None):
        """configs[3] through the graph object (include/hmsg.h: hmsg_graph_allgather_index): the ranks' node tables AND the levels above
        them -- floors -> rooms, room keys, view embeddings, room names -- into one resident index per rank, global ids throughout.
        -> (NodeIndex, node_off, room_off, floor_off), offsets [world + 1]."""
        ix = _P()
        rn = None if room_name_emb is None else np.ascontiguousarray(np.asarray(room_name_emb, np.float64))
        noff, roff, foff = (np.zeros(comm.world + 1, np.int64) for _ in range(3))
        self._ck(self.L.c.hmsg_graph_allgather_index(self.g, comm.h, None if rn is None else _ptr(rn), C.byref(ix), _ptr(noff), _ptr(roff), _ptr(foff)))
        nx = NodeIndex._wrap(self.L, ix, int(noff[-1]), self.D)
        nx._n_rooms = int(roff[-1])
        return nx, noff, roff, foff

    def name_rooms(self, method, type_feats, type_names):
        """hmsg_graph_name_rooms: Graph.generate_room_names(generate_method=method, default_room_types=type_names) with
        type_feats = the types' text features; method "obj_embedding" or "view_embedding".  -> chosen type per room (-1: unchanged)."""
        m = {"obj_embedding": ROOM_NAMES_OBJ_EMBEDDING, "view_embedding": ROOM_NAMES_VIEW_EMBEDDING}[method]
        T = np.ascontiguousarray(np.asarray(type_feats, np.float32))
        names, keep = self._strs(type_names)
        assert T.ndim == 2 and len(T) == len(type_names)
        out = np.full(max(self.counts()["rooms"], 1), -1, np.int32)
        self._ck(self.L.c.hmsg_graph_name_rooms(self.g, m, len(T), _ptr(T), C.cast(names, _P), _ptr(out)))
        return out[: self.counts()["rooms"]]

    def set_room_names(self, names):
        """hmsg_graph_set_room_names (Graph.set_room_names)"""
        arr, keep = self._strs(names)
        self._ck(self.L.c.hmsg_graph_set_room_names(self.g, len(names), C.cast(arr, _P)))

    def query(self, T_obj, qid, T_room, floor_id, room_mode, k, use_negatives=True, room_name_emb=None, max_rooms=None):
        """hmsg_graph_query: floor -> room(s) -> objects on the graph's own index (made on the first call)"""
        T_obj = np.ascontiguousarray(T_obj, dtype=np.float32)
        Q, Cn, D = T_obj.shape
        T_room = None if T_room is None else np.ascontiguousarray(T_room, dtype=np.float32)
        qid = np.ascontiguousarray(qid, dtype=np.int32)
        floor_id = np.ascontiguousarray(floor_id, dtype=np.int32)
        room_mode = np.ascontiguousarray(room_mode, dtype=np.int32)
        rn = None if room_name_emb is None else np.ascontiguousarray(np.asarray(room_name_emb, np.float64))
        RM = int(max_rooms or max(self.counts()["rooms"], 10))
        sel, nsel = np.empty((Q, RM), np.int32), np.empty((Q,), np.int32)
        idx, room, score = np.empty((Q, k), np.int32), np.empty((Q, k), np.int32), np.empty((Q, k), np.float64)
        self._ck(self.L.c.hmsg_graph_query(self.g, None if rn is None else _ptr(rn), Q, Cn, _ptr(T_obj), _ptr(qid),
                                           None if T_room is None else _ptr(T_room), _ptr(floor_id), _ptr(room_mode), int(k), int(use_negatives), RM,
                                           _ptr(sel), _ptr(nsel), _ptr(idx), _ptr(room), _ptr(score)))
        return [sel[q, : nsel[q]].tolist() for q in range(Q)], idx, room, score

    # ---- the view level of the slow path (include/hmsg.h: Graph.query_room_obj_slow_reasoning between its VLM calls)
    def views(self):
        n = self.counts()["views"]
        arr = (HmsgGraphView * max(n, 1))()
        self._ck(self.L.c.hmsg_graph_get_views(self.g, C.cast(arr, _P), n))
        return [dict(view=a.view, room=a.room, img_id=a.img_id, n_objects=a.n_objects) for a in arr[:n]]

    def view_objects(self, view, n=None):
        n = int(n if n is not None else self.views()[view]["n_objects"])
        out = np.zeros(max(n, 1), np.int32)
        self._ck(self.L.c.hmsg_graph_get_view_objects(self.g, int(view), _ptr(out), n))
        return out[:n]

    def find_view(self, img_path=None, img_id=-1):
        """find_view_by_imgpath: by path when given, otherwise by image id; -1 when there is none"""
        v = C.c_int32(-1)
        self._ck(self.L.c.hmsg_graph_find_view(self.g, None if img_path is None else str(img_path).encode(), int(img_id), C.byref(v)))
        return v.value

    def object_best_views(self, objs):
        objs = np.ascontiguousarray(objs, dtype=np.int32)
        view, img = np.full(max(len(objs), 1), -1, np.int32), np.full(max(len(objs), 1), -1, np.int64)
        self._ck(self.L.c.hmsg_graph_object_best_views(self.g, len(objs), _ptr(objs), _ptr(view), _ptr(img)))
        return view[: len(objs)], img[: len(objs)]

    def goal_views(self, T, floor_id, k=24):
        """hmsg_graph_goal_views -> (img ids [Q][k], rooms [Q][k], scores [Q][k], counts [Q]); -1 / -1 / 0.0 past the count"""
        T = np.ascontiguousarray(T, dtype=np.float32)
        Q = len(T)
        floor_id = np.ascontiguousarray(floor_id, dtype=np.int32)
        assert T.ndim == 2 and floor_id.shape == (Q,)
        img, room = np.empty((Q, k), np.int64), np.empty((Q, k), np.int32)
        score, n = np.empty((Q, k), np.float64), np.empty((Q,), np.int32)
        self._ck(self.L.c.hmsg_graph_goal_views(self.g, Q, _ptr(T), _ptr(floor_id), int(k), _ptr(img), _ptr(room), _ptr(score), _ptr(n)))
        return img, room, score, n

    def rematch_in_views(self, T, view, pose_inv=None, wh=None, K=None):
        """hmsg_graph_rematch_in_views -> (object index [Q], score [Q], avg distance [Q] or None)"""
        T = np.ascontiguousarray(T, dtype=np.float32)
        Q = len(T)
        view = np.ascontiguousarray(view, dtype=np.int32)
        assert T.ndim == 2 and view.shape == (Q,)
        obj, score = np.empty((Q,), np.int32), np.empty((Q,), np.float64)
        Pi = dist = whp = Kp = None
        if pose_inv is not None:
            Pi = np.ascontiguousarray(np.asarray(pose_inv, np.float64).reshape(Q, 16))
            whp = np.ascontiguousarray(np.broadcast_to(np.asarray(wh, np.int32), (Q, 2)))
            Kp = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
            dist = np.empty((Q,), np.float64)
        self._ck(self.L.c.hmsg_graph_rematch_in_views(self.g, Q, _ptr(T), _ptr(view), _ptr(Pi), _ptr(whp), _ptr(Kp), _ptr(obj), _ptr(score), _ptr(dist)))
        return obj, score, dist

    def object_view_depths(self, objs, pose_inv, wh, K):
        """hmsg_graph_object_view_depths: check_object_in_view(..., return_depth=True) -> (visible bool [n], mean_depth [n])"""
        objs = np.ascontiguousarray(objs, dtype=np.int32)
        n = len(objs)
        Pi = np.ascontiguousarray(np.asarray(pose_inv, np.float64).reshape(n, 16))
        whp = np.ascontiguousarray(np.broadcast_to(np.asarray(wh, np.int32), (n, 2)))
        Kp = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
        vis, md = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.float64)
        self._ck(self.L.c.hmsg_graph_object_view_depths(self.g, n, _ptr(objs), _ptr(Pi), _ptr(whp), _ptr(Kp), _ptr(vis), _ptr(md)))
        return vis[:n].astype(bool), md[:n]

    def query_sharded(self, comm: "Comm", T_obj, qid, T_room, floor_id, room_mode, k, use_negatives=True, room_name_emb=None, max_rooms=None):
        """hmsg_graph_query_sharded: one call per rank with the same queries; the answer of hmsg_query_hier on the concatenated tables,
        on every rank, with no table gathered.  -> (sel, idx, room, score, node_off, room_off, floor_off), offsets [world + 1]."""
        rn = None if room_name_emb is None else np.ascontiguousarray(np.asarray(room_name_emb, np.float64))
        if max_rooms is None:       # max(rooms of ALL ranks, 10), as the concatenated index's query_hier: the header exchange alone (Q = 0)
            roff = np.zeros(comm.world + 1, np.int64)
            self._ck(self.L.c.hmsg_graph_query_sharded(self.g, comm.h, None if rn is None else _ptr(rn), 0, 1, None, None, None, None, None, 1,
                                                       int(use_negatives), 1, None, None, None, None, None, None, _ptr(roff), None))
            max_rooms = max(int(roff[-1]), 10)
        a = _sharded_args(T_obj, qid, T_room, floor_id, room_mode, k, max_rooms, comm.world)
        self._ck(self.L.c.hmsg_graph_query_sharded(self.g, comm.h, None if rn is None else _ptr(rn), *a["args"], int(use_negatives),
                                                   *a["outs"]))
        return a["result"]()


def _sharded_args(T_obj, qid, T_room, floor_id, room_mode, k, max_rooms, n):
    """the query arguments and output arrays of hmsg_graph_query_sharded / hmsg_graphs_query (use_negatives goes between them)"""
    T_obj = np.ascontiguousarray(T_obj, dtype=np.float32)
    Q, Cn, D = T_obj.shape
    T_room = None if T_room is None else np.ascontiguousarray(T_room, dtype=np.float32)
    qid = np.ascontiguousarray(qid, dtype=np.int32)
    floor_id = np.ascontiguousarray(floor_id, dtype=np.int32)
    room_mode = np.ascontiguousarray(room_mode, dtype=np.int32)
    RM, k = int(max_rooms), int(k)
    sel, nsel = np.empty((Q, RM), np.int32), np.zeros((Q,), np.int32)
    idx, room, score = np.empty((Q, k), np.int32), np.empty((Q, k), np.int32), np.empty((Q, k), np.float64)
    noff, roff, foff = (np.zeros(n + 1, np.int64) for _ in range(3))
    keep = (T_obj, T_room, qid, floor_id, room_mode)
    args = (Q, Cn, _ptr(T_obj), _ptr(qid), None if T_room is None else _ptr(T_room), _ptr(floor_id), _ptr(room_mode), k)
    outs = (RM, _ptr(sel), _ptr(nsel), _ptr(idx), _ptr(room), _ptr(score), _ptr(noff), _ptr(roff), _ptr(foff))
    return dict(keep=keep, args=args, outs=outs,
                result=lambda: ([sel[q, : nsel[q]].tolist() for q in range(Q)], idx, room, score, noff, roff, foff))


def query_graphs(graphs, room_name_embs, T_obj, qid, T_room, floor_id, room_mode, k, use_negatives=True, max_rooms=None):
    """hmsg_graphs_query: the sharded query over several SceneGraphs held by this process on one device (a multi-building service):
    the answer of hmsg_query_hier on the concatenated tables, with no concatenated table.  room_name_embs: one f64 [R_i, D] per graph,
    or None (no label mode).  -> (sel, idx, room, score, node_off, room_off, floor_off), offsets [len(graphs) + 1]."""
    graphs = list(graphs)
    n = len(graphs)
    assert n >= 1
    L = graphs[0].L
    if max_rooms is None:
        max_rooms = max(sum(g.counts()["rooms"] for g in graphs), 10)
    a = _sharded_args(T_obj, qid, T_room, floor_id, room_mode, k, max_rooms, n)
    gs = (_P * n)(*[g.g for g in graphs])
    rns = None
    if room_name_embs is not None:
        rn = [None if r is None else np.ascontiguousarray(np.asarray(r, np.float64)) for r in room_name_embs]
        assert len(rn) == n
        rns = (_P * n)(*[None if r is None else r.ctypes.data for r in rn])
    rc = L.c.hmsg_graphs_query(n, C.cast(gs, _P), None if rns is None else C.cast(rns, _P), *a["args"], int(use_negatives), *a["outs"])
    if rc != 0:
        raise HmsgError(L.c.hmsg_graph_last_error(graphs[0].g).decode() + f" (rc={rc})")
    return a["result"]()


def sharded_query_bytes(world, Q, k, rooms, floors, floor_rooms, label=True, view=False):
    """bytes ONE rank receives per hmsg_graph_query_sharded call (include/hmsg.h): its header, room and candidate all-gathers, its own
    slots included; summed over the ranks the traffic is about `world` times this.  rooms / floors / floor_rooms: the largest count of
    any rank."""
    a16 = lambda b: (b + 15) // 16 * 16
    R, F, FR = max(rooms, 1), max(floors, 1), max(floor_rooms, 1)
    room = (a16(Q * R * 8) if label else 0) + (a16(Q * R * 8) if view else 0) + a16(4 * (F + 1)) + a16(4 * FR) + 2 * a16(4 * R)
    cand = a16(Q * 2 * k * 24) + a16(Q * 4)
    return world * (128 + room + cand)


ROOM_NAMES_OBJ_EMBEDDING, ROOM_NAMES_VIEW_EMBEDDING = 1, 2     # include/hmsg.h: HMSG_ROOM_NAMES_*


def points_view_depths(clouds, pose_inv, wh, K, min_visible_ratio=0.5, max_depth=10.0, device_id=0, lib_: "HmsgLib | None" = None):
    """hmsg_points_view_depths: cloud p (float64 [n][3]) through camera p -> (avg_z_front [P] (NaN: no point in front of the camera),
    visible bool [P], mean_depth [P] (inf as check_object_in_view returns it))"""
    L = lib_ or lib()
    P = len(clouds)
    off = np.zeros(P + 1, np.int64)
    for i, c in enumerate(clouds):
        off[i + 1] = off[i] + len(c)
    pts = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in clouds], 0)) if P else np.zeros((0, 3))
    if not len(pts):
        pts = np.zeros((1, 3), np.float64)
    Pi = np.ascontiguousarray(np.asarray(pose_inv, np.float64).reshape(max(P, 0), 16))
    whp = np.ascontiguousarray(np.broadcast_to(np.asarray(wh, np.int32), (P, 2)))
    Kp = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
    avg, vis, md = np.zeros(max(P, 1), np.float64), np.zeros(max(P, 1), np.uint8), np.zeros(max(P, 1), np.float64)
    rc = L.c.hmsg_points_view_depths(int(device_id), P, _ptr(off), _ptr(pts), _ptr(Pi), _ptr(whp), _ptr(Kp), float(min_visible_ratio), float(max_depth),
                                     _ptr(avg), _ptr(vis), _ptr(md))
    if rc != 0:
        raise HmsgError(f"hmsg_points_view_depths failed ({rc})")
    return avg[:P], vis[:P].astype(bool), md[:P]


def denoise_feats_batch(sets, eps=0.02, min_samples=2, device_id=0, lib_: "HmsgLib | None" = None):
    """feats_denoise_dbscan (utils/graph_utils.py:682-728) of many sets at once on the device (include/hmsg.h:
    hmsg_denoise_feats_batch).  sets: arrays [n_k, D], all float32 or all float64 (np.array of the rows, as the reference
    takes them).  -> (representatives [K, D] in that dtype, rows of the chosen cluster per set, 0 = no cluster)."""
    L = lib_ or lib()
    rows = [np.asarray(s_) for s_ in sets]
    K = len(rows)
    f64 = any(r.dtype != np.float32 for r in rows)
    dt = np.float64 if f64 else np.float32
    D = next((r.reshape(len(r), -1).shape[1] for r in rows if r.size), 0)
    rows = [r.reshape(len(r), D) if r.size else np.zeros((0, D), dt) for r in rows]
    off = np.zeros(K + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    X = np.ascontiguousarray(np.concatenate(rows).astype(dt, copy=False) if K and off[-1] else np.zeros((1, max(D, 1)), dt))
    out = np.zeros((K, D), dt)
    ncl = np.zeros(K, np.int32)
    if K == 0:
        return out, ncl
    rc = L.c.hmsg_denoise_feats_batch(int(device_id), K, _ptr(off), _ptr(X), int(f64), int(D), float(eps), int(min_samples), _ptr(out), _ptr(ncl))
    if rc != 0:
        bad = [k for k in range(K) if off[k + 1] == off[k]]
        raise HmsgError(f"hmsg_denoise_feats_batch failed ({rc})" + (f": set {bad[0]} is empty" if bad else ""))
    return out, ncl


def points_min_dist_2d(sets, queries, device_id=0, lib_: "HmsgLib | None" = None):
    """out[q][s] = np.min(cdist([queries[q]], sets[s], "euclidean")) on the device (camera -> room assignment of
    compute_room_embeddings, utils/graph_utils.py:244-291)."""
    L = lib_ or lib()
    off = np.zeros(len(sets) + 1, np.int64)
    off[1:] = np.cumsum([len(s_) for s_ in sets])
    pts = np.ascontiguousarray(np.concatenate([np.asarray(s_, np.float64).reshape(-1, 2) for s_ in sets])
                               if off[-1] else np.zeros((1, 2)), dtype=np.float64)
    q = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 2)
    out = np.full((len(q), len(sets)), np.inf)
    rc = L.c.hmsg_points_min_dist_2d(device_id, len(sets), _ptr(off), _ptr(pts), len(q), _ptr(q), _ptr(out))
    if rc != 0:
        raise HmsgError(f"hmsg_points_min_dist_2d failed ({rc})")
    return out


def lidar_depth(clouds, poses, intrinsics, width, height, voxel_size=0.02, depth_factor=1000.0, image_scale=1,
                want_state=False, device_id=0, lib_: "HmsgLib | None" = None):
    """LiDAR local maps -> occlusion-aware uint16 depth images on the device (include/hmsg.h: hmsg_lidar_depth; the
    reference's generate_depth.py process_frame per frame).  `clouds`: one [n_f, 3] float64 array per frame; `poses`:
    [F, 3, 4] world -> camera [R | t], or None when the clouds already hold (u, v, z) rows; `intrinsics`: 3x3 K.
    Returns (depth [F, H, W] uint16, stats [F, 4] int64, state per input point or None, device milliseconds)."""
    L = lib_ or lib()
    F = len(clouds)
    off = np.zeros(F + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in clouds])
                               if off[-1] else np.zeros((1, 3)), dtype=np.float64)
    K = np.asarray(intrinsics, np.float64)
    prm = HmsgDepthParams(int(width), int(height), int(image_scale), K[0, 0], K[1, 1], K[0, 2], K[1, 2], float(voxel_size),
                          float(depth_factor))
    T = None
    if poses is not None:
        P = np.asarray(poses, np.float64).reshape(F, 3, 4)
        T = np.ascontiguousarray(np.concatenate([P[:, :, :3].reshape(F, 9), P[:, :, 3]], axis=1))
    depth = np.zeros((F, int(height), int(width)), np.uint16)
    stats = np.zeros((F, 4), np.int64)
    state = np.zeros(max(int(off[-1]), 1), np.uint8) if want_state else None
    ms = C.c_double(0.0)
    rc = L.c.hmsg_lidar_depth(device_id, C.byref(prm), F, _ptr(pts), _ptr(off), _ptr(T) if T is not None else None,
                              _ptr(depth), _ptr(state) if state is not None else None, _ptr(stats), C.byref(ms))
    if rc != 0:
        raise HmsgError(f"hmsg_lidar_depth failed ({rc})")
    return depth, stats, (state[:int(off[-1])] if state is not None else None), ms.value


def write_json_record(path, fields, lib_: "HmsgLib | None" = None):
    """One node record of the on-disk graph through the C ABI (include/hmsg.h: hmsg_write_json) -- byte for byte json.dump's
    text.  fields: (key, value) pairs in the reference's key order; a numpy array of floats (float32 / float64, up to 2-D) or
    of ints is printed by the library, a Python float likewise; everything else (str, None, lists of ids / strings / ints,
    ragged things) goes through json.dumps here and travels as RAW text."""
    import json
    L = lib_ or lib()
    keep, arr = [], (HmsgJsonField * max(len(fields), 1))()
    for k, (key, v) in enumerate(fields):
        f = arr[k]
        f.key = key.encode()
        if isinstance(v, np.ndarray) and v.ndim <= 2 and v.dtype in (np.float64, np.float32) or \
                (isinstance(v, np.ndarray) and v.ndim <= 2 and np.issubdtype(v.dtype, np.integer)):
            if np.issubdtype(v.dtype, np.integer):
                a, kind = np.ascontiguousarray(v, np.int64), 3
            else:
                a, kind = np.ascontiguousarray(v), (1 if v.dtype == np.float64 else 2)
            keep.append(a)
            f.kind, f.ndim = kind, a.ndim
            f.n0 = a.shape[0] if a.ndim >= 1 else 0
            f.n1 = a.shape[1] if a.ndim == 2 else 0
            f.data = a.ctypes.data if a.size else None
        elif isinstance(v, float):
            a = np.array([v], np.float64)
            keep.append(a)
            f.kind, f.ndim, f.n0, f.n1, f.data = 1, 0, 0, 0, a.ctypes.data
        else:
            raw = json.dumps(v).encode()
            keep.append(raw)
            f.kind, f.ndim, f.n0, f.n1 = 0, 0, 0, 0
            f.data = C.cast(C.c_char_p(raw), C.c_void_p)
    rc = L.c.hmsg_write_json(str(path).encode(), len(fields), C.cast(arr, _P))
    if rc != 0:
        raise HmsgError(f"hmsg_write_json failed ({rc}) for {path}")


def write_ply(path, pts, lib_: "HmsgLib | None" = None):
    """A cloud as Open3D's write_point_cloud writes it (include/hmsg.h: hmsg_write_ply)."""
    L = lib_ or lib()
    a = np.ascontiguousarray(np.asarray(pts, np.float64).reshape(-1, 3))
    rc = L.c.hmsg_write_ply(str(path).encode(), _ptr(a) if a.size else None, a.shape[0])
    if rc != 0:
        raise HmsgError(f"hmsg_write_ply failed ({rc}) for {path}")


def read_json_numbers(path, key, lib_: "HmsgLib | None" = None):
    """The numbers under `key` of a saved node record, flattened (include/hmsg.h: hmsg_read_json_numbers)."""
    L = lib_ or lib()
    n = C.c_int64(0)
    rc = L.c.hmsg_read_json_numbers(str(path).encode(), key.encode(), None, 0, C.byref(n))
    if rc != 0:
        raise HmsgError(f"hmsg_read_json_numbers failed ({rc}) for {key} of {path}")
    out = np.empty(max(n.value, 1), np.float64)
    rc = L.c.hmsg_read_json_numbers(str(path).encode(), key.encode(), _ptr(out), n.value, C.byref(n))
    if rc != 0:
        raise HmsgError(f"hmsg_read_json_numbers failed ({rc}) for {key} of {path}")
    return out[: n.value]


def assign_cameras_to_rooms(dist, cam_height, y_min, y_max, lib_: "HmsgLib | None" = None):
    """compute_room_embeddings' camera -> room step (include/hmsg.h: hmsg_assign_cameras_to_rooms).  dist [n_cams, n_rooms].
    Returns (room_of_cam [n_cams] int32, per-room image id lists)."""
    L = lib_ or lib()
    d = np.ascontiguousarray(np.asarray(dist, np.float64))
    n_cams, n_rooms = (int(d.shape[0]), int(d.shape[1])) if d.ndim == 2 else (0, 0)
    h = np.ascontiguousarray(np.asarray(cam_height, np.float64).reshape(-1))
    room_of = np.full(max(n_cams, 1), -1, np.int32)
    off = np.zeros(n_rooms + 1, np.int64)
    imgs = np.zeros(max(n_cams + n_rooms, 1), np.int32)
    rc = L.c.hmsg_assign_cameras_to_rooms(_ptr(d) if d.size else None, n_cams, n_rooms, _ptr(h) if h.size else None, float(y_min),
                                          float(y_max), _ptr(room_of), _ptr(off), _ptr(imgs))
    if rc != 0:
        raise HmsgError(f"hmsg_assign_cameras_to_rooms failed ({rc})")
    return room_of[:n_cams], [imgs[off[r]:off[r + 1]].tolist() for r in range(n_rooms)]


def kmeans(X, n_clusters, n_init=5, max_iter=100, seed=0, lib_: "HmsgLib | None" = None):
    """KMeans(n_clusters, n_init, max_iter, random_state=seed).fit(X) behind the C ABI (include/hmsg.h: hmsg_kmeans; a restatement
    of scikit-learn's Lloyd KMeans for hosts without it).  Returns (labels i32 [n], centers f32 [k, D], inertia, n_iter)."""
    L = lib_ or lib()
    X = np.ascontiguousarray(np.asarray(X, np.float32))
    n, D = X.shape
    labels = np.empty(n, np.int32)
    centers = np.empty((int(n_clusters), D), np.float32)
    inertia, n_iter = C.c_float(0), C.c_int32(0)
    rc = L.c.hmsg_kmeans(_ptr(X), n, D, int(n_clusters), int(n_init), int(max_iter), int(seed), _ptr(labels), _ptr(centers),
                         C.byref(inertia), C.byref(n_iter))
    if rc != 0:
        raise HmsgError(f"hmsg_kmeans failed ({rc})")
    return labels, centers, float(inertia.value), int(n_iter.value)


def kmeans_batch(sets, n_clusters, n_init=5, max_iter=100, seed=0, lib_: "HmsgLib | None" = None):
    """hmsg_kmeans for several independent sets in one call, on the device (include/hmsg.h: hmsg_kmeans_batch): the bits of
    kmeans(set, ...) per set.  `sets`: float32 arrays [n_s, D], or torch tensors on the device (the results are device tensors
    then).  Returns a list of (labels i32 [n_s], centers f32 [k, D], inertia, n_iter), one per set."""
    L = lib_ or lib()
    sets = list(sets)
    if not sets:
        return []
    k = int(n_clusters)
    on_dev = all(hasattr(x, "data_ptr") and getattr(x, "is_cuda", False) for x in sets)
    if on_dev:
        import torch
        dev = sets[0].device
        X = torch.cat([x.to(torch.float32).reshape(x.shape[0], -1) for x in sets], 0).contiguous()
        D, device_id = int(X.shape[1]), dev.index or 0
        sizes = [int(x.shape[0]) for x in sets]
        labels = torch.empty(sum(sizes), dtype=torch.int32, device=dev)
        centers = torch.empty((len(sets), k, D), dtype=torch.float32, device=dev)
    else:
        rows = [np.ascontiguousarray(np.asarray(x.cpu() if hasattr(x, "cpu") else x, np.float32)) for x in sets]
        rows = [x.reshape(x.shape[0], -1) for x in rows]
        X = np.ascontiguousarray(np.concatenate(rows, 0))
        D, device_id = int(X.shape[1]), 0
        sizes = [int(x.shape[0]) for x in rows]
        labels = np.empty(sum(sizes), np.int32)
        centers = np.empty((len(sets), k, D), np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    inertia, n_iter = np.zeros(len(sets), np.float32), np.zeros(len(sets), np.int32)
    rc = L.c.hmsg_kmeans_batch(device_id, len(sets), _ptr(off), _ptr(X), D, k, int(n_init), int(max_iter), int(seed), _ptr(labels),
                               _ptr(centers), _ptr(inertia), _ptr(n_iter))
    if rc != 0:
        raise HmsgError(f"hmsg_kmeans_batch failed ({rc})")
    return [(labels[off[s]:off[s + 1]], centers[s], float(inertia[s]), int(n_iter[s])) for s in range(len(sets))]


def pick_representative_views(embs, labels, centers, lib_: "HmsgLib | None" = None):
    """Per KMeans label present (ascending), the member closest (dot product) to its centre (include/hmsg.h:
    hmsg_pick_representative_views).  Returns indices into the room's image list."""
    L = lib_ or lib()
    e = np.ascontiguousarray(np.asarray(embs, np.float32))
    c = np.ascontiguousarray(np.asarray(centers, np.float32))
    lab = np.ascontiguousarray(np.asarray(labels, np.int32).reshape(-1))
    out = np.zeros(max(c.shape[0], 1), np.int32)
    n = C.c_int32(0)
    rc = L.c.hmsg_pick_representative_views(_ptr(e) if e.size else None, e.shape[0], e.shape[1], _ptr(lab) if lab.size else None,
                                            _ptr(c) if c.size else None, c.shape[0], _ptr(out), C.byref(n))
    if rc != 0:
        raise HmsgError(f"hmsg_pick_representative_views failed ({rc})")
    return out[: n.value].tolist()


def graph_edges(n_floors, room_floor, obj_room, view_room, view_objs, lib_: "HmsgLib | None" = None):
    """create_graph_new as an edge list of node ids (0 building, floors, rooms, objects, views; include/hmsg.h:
    hmsg_graph_edges).  view_objs: per view, the positions of its objects.  Returns int64 [n_edges, 2]."""
    L = lib_ or lib()
    rf = np.ascontiguousarray(np.asarray(room_floor, np.int32).reshape(-1))
    orm = np.ascontiguousarray(np.asarray(obj_room, np.int32).reshape(-1))
    vr = np.ascontiguousarray(np.asarray(view_room, np.int32).reshape(-1))
    off = np.zeros(len(vr) + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v in view_objs]) if len(vr) else 0
    vo = np.ascontiguousarray(np.asarray([o for v in view_objs for o in v], np.int32))
    cap = 1 + int(n_floors) + len(rf) + len(orm) + len(vr) + len(vo)
    edges = np.zeros((max(cap, 1), 2), np.int64)
    n = C.c_int64(0)
    rc = L.c.hmsg_graph_edges(int(n_floors), len(rf), _ptr(rf) if rf.size else None, len(orm), _ptr(orm) if orm.size else None, len(vr),
                              _ptr(vr) if vr.size else None, _ptr(off), _ptr(vo) if vo.size else None, _ptr(edges), cap, C.byref(n))
    if rc != 0:
        raise HmsgError(f"hmsg_graph_edges failed ({rc})")
    return edges[: n.value]


def crop_all_bounding_boxs(image, masks, bbox_margin=0, size=512, plain=True, masked=True, device_id=0,
                           lib_: "HmsgLib | None" = None):
    """Both crop sets of one frame on the device (include/hmsg.h: hmsg_crop_resize_batch; utils/sam_utils.py:119-147 as
    called by sam_clip_feats_extractor.py:148-151).  `masks`: SAM records (dicts with "segmentation" and "bbox" XYWH).
    Returns (plain [M, S, S, 3] uint8 or None, masked [M, S, S, 3] uint8 or None)."""
    L = lib_ or lib()
    image = np.ascontiguousarray(image, dtype=np.uint8)
    H, W = image.shape[:2]
    M = len(masks)
    bbox = np.ascontiguousarray([m["bbox"] for m in masks], dtype=np.float64).reshape(M, 4)
    segs = np.ascontiguousarray(np.stack([m["segmentation"] for m in masks]).astype(np.uint8)) if (masked and M) else None
    o_plain = np.zeros((M, size, size, 3), np.uint8) if plain else None
    o_masked = np.zeros((M, size, size, 3), np.uint8) if masked else None
    rc = L.c.hmsg_crop_resize_batch(device_id, H, W, _ptr(image), M, _ptr(segs), _ptr(bbox), float(bbox_margin), int(size),
                                    _ptr(o_plain), _ptr(o_masked), None)
    if rc != 0:
        raise HmsgError(f"hmsg_crop_resize_batch failed ({rc})")
    return o_plain, o_masked


def _rle_one_frame(fn, rles, H, W, out_dtype, device_id, lib_):
    L = lib_ or lib()
    if isinstance(rles, list):
        from . import rle as _rle
        counts, run_off, _ = _rle.pack([rles])
    else:
        counts, run_off = rles[0], rles[1]
    on_dev = hasattr(counts, "data_ptr") and getattr(counts, "is_cuda", False)
    if not on_dev:
        counts, run_off = np.ascontiguousarray(counts, dtype=np.uint32), np.ascontiguousarray(run_off, dtype=np.int64)
    M = int(run_off.shape[0]) - 1
    NW = (max(M, 1) + 63) // 64
    shape = (H * W, NW) if out_dtype == "bits" else (M, H, W)
    if on_dev:
        import torch
        device_id = counts.device.index or 0
        # (torch has no uint64 arithmetic: the words travel as int64 with the same bits)
        out = torch.empty(shape, dtype=torch.int64 if out_dtype == "bits" else torch.uint8, device=counts.device)
    else:
        out = np.empty(shape, np.uint64 if out_dtype == "bits" else np.uint8)
    rc = getattr(L.c, fn)(int(device_id), int(H), int(W), M, _ptr(counts) if M else None, _ptr(run_off), _ptr(out) if int(np.prod(shape)) else None)
    if rc != 0:
        raise HmsgError(f"{fn} failed ({rc}): malformed run-length masks (the message is on stderr)")
    return out


def rle_to_bitsets(rles, H, W, device_id=0, lib_: "HmsgLib | None" = None):
    """One frame's run-length masks -> per-pixel membership bitsets [H * W, NW] (include/hmsg.h: hmsg_rle_to_bitsets): bit i & 63
    of word i >> 6 of pixel y * W + x says that mask i covers it.  rles: a list of counts (one per mask) or (counts, run_off) as
    rle.pack makes them, numpy arrays (returns numpy uint64) or torch device tensors (returns a device tensor, int64 bits)."""
    return _rle_one_frame("hmsg_rle_to_bitsets", rles, H, W, "bits", device_id, lib_)


def rle_to_masks(rles, H, W, device_id=0, lib_: "HmsgLib | None" = None):
    """One frame's run-length masks -> dense uint8 [M, H, W] (0 / 1) made on the device (include/hmsg.h: hmsg_rle_to_masks): with
    device tensors in, the dense masks the crop calls read never exist on the host.  rles as in rle_to_bitsets."""
    return _rle_one_frame("hmsg_rle_to_masks", rles, H, W, "masks", device_id, lib_)


def sam_post_params(lib_: "HmsgLib | None" = None, **over):
    """hmsg_sam_post_params with SAM's defaults (hmsg_sam_post_default_params), fields overridden by keyword"""
    L = lib_ or lib()
    p = HmsgSamPostParams()
    L.c.hmsg_sam_post_default_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise HmsgError(f"unknown hmsg_sam_post_params field {k}")
        setattr(p, k, int(v) if k == "min_mask_region_area" else float(v))
    return p


def sam_postprocess(logits, iou_preds, params=None, max_out=None, counts_cap=None, return_masks=True, device_id=0,
                    lib_: "HmsgLib | None" = None, **over):
    """SAM's mask post-processing on the device (include/hmsg.h: hmsg_sam_postprocess): logits float32 [N, H, W] (or [P, 3, H, W]) and
    iou_preds float32 [N] (or [P, 3]) as predict_torch(..., return_logits=True) returns them -> a dict with n, keep_idx [n], counts,
    run_off [n + 1] (the records of hmsg_add_frame_features_rle), bbox [n, 4] float64 XYWH, area [n], stability_score [n], masks
    uint8 [n, H, W] (with return_masks), device_ms.  numpy arrays in: numpy arrays out; torch device tensors in: the outputs are
    device tensors (counts as int32 with uint32's bits), no mask or record crosses to the host.  params: an HmsgSamPostParams, or
    fields by keyword (pred_iou_thresh=..., min_mask_region_area=...).  max_out / counts_cap size the output arrays (default: min(N,
    256) masks and two counts per mask and column); when the library asks for more the call is repeated once with what it asked for."""
    L = lib_ or lib()
    prm = params if params is not None else sam_post_params(L, **over)
    on_dev = hasattr(logits, "data_ptr") and getattr(logits, "is_cuda", False)
    if on_dev:
        import torch
        assert logits.dtype == torch.float32 and iou_preds.dtype == torch.float32 and iou_preds.device == logits.device
        logits, iou_preds = logits.contiguous(), iou_preds.contiguous()
        device_id = logits.device.index or 0
    else:
        logits, iou_preds = np.ascontiguousarray(logits, dtype=np.float32), np.ascontiguousarray(iou_preds, dtype=np.float32)
    H, W = (int(v) for v in logits.shape[-2:])
    N = int(np.prod(tuple(logits.shape[:-2]))) if len(logits.shape) > 2 else 1
    assert int(np.prod(tuple(iou_preds.shape))) == N, "iou_preds: one value per logit image"
    if N == 0 and on_dev:                                   # (an empty tensor has no address; the library wants one and reads nothing)
        logits, iou_preds = logits.new_zeros(1), iou_preds.new_zeros(1)
    cap_m = int(max_out) if max_out is not None else min(max(N, 1), 256)
    cap_c = int(counts_cap) if counts_cap is not None else cap_m * (2 * W + 2) + 64
    for attempt in range(2):
        def buf(shape, np_dtype, t_dtype):
            if on_dev:
                return torch.empty(shape, dtype=getattr(torch, t_dtype), device=logits.device)
            return np.empty(shape, np_dtype)
        keep, counts, run_off = buf((cap_m,), np.int32, "int32"), buf((max(cap_c, 1),), np.uint32, "int32"), buf((cap_m + 1,), np.int64, "int64")
        bbox, area, stab = buf((cap_m, 4), np.float64, "float64"), buf((cap_m,), np.int32, "int32"), buf((cap_m,), np.float32, "float32")
        masks = buf((max(cap_m, 1), H, W), np.uint8, "uint8") if return_masks else None
        n, nc, ms = C.c_int32(0), C.c_int64(0), C.c_double(0.0)
        rc = L.c.hmsg_sam_postprocess(int(device_id), C.byref(prm), N, H, W, _ptr(logits), _ptr(iou_preds), cap_m, cap_c, C.byref(n),
                                      C.byref(nc), _ptr(keep), _ptr(counts), _ptr(run_off), _ptr(bbox), _ptr(area), _ptr(stab), _ptr(masks),
                                      C.byref(ms))
        if rc == 0:
            break
        if attempt == 0 and rc == -1 and (n.value > cap_m or nc.value > cap_c):
            cap_m, cap_c = max(cap_m, n.value), max(cap_c, nc.value)
            continue
        raise HmsgError(f"hmsg_sam_postprocess failed ({rc}) (the message is on stderr)")
    k = n.value
    return dict(n=k, keep_idx=keep[:k], counts=counts[:nc.value], run_off=run_off[:k + 1], bbox=bbox[:k], area=area[:k],
                stability_score=stab[:k], masks=masks[:k] if return_masks else None, device_ms=ms.value, size=(H, W))


def nav_params(lib_: "HmsgLib | None" = None, **over):
    """hmsg_nav_params with the reference's values (hmsg_nav_default_params), fields overridden by keyword"""
    L = lib_ or lib()
    p = HmsgNavParams()
    L.c.hmsg_nav_default_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise HmsgError(f"unknown hmsg_nav_params field {k}")
        setattr(p, k, int(v) if k in ("dilation", "blur", "pose_min_samples", "region_rule") else float(v))
    return p


def nav_grid(points, cell_size=0.03, device_id=0, lib_: "HmsgLib | None" = None):
    """bounds and grid of a storey's cloud (include/hmsg.h: hmsg_nav_grid): points float64 [n, 3], numpy or a device tensor
    -> (pcd_min [3], pcd_max [3], (columns, rows))"""
    L = lib_ or lib()
    if not (hasattr(points, "data_ptr") and getattr(points, "is_cuda", False)):
        points = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    mn, mx, grid = np.zeros(3), np.zeros(3), np.zeros(2, np.int32)
    rc = L.c.hmsg_nav_grid(int(device_id), float(cell_size), int(points.shape[0]), _ptr(points), _ptr(mn), _ptr(mx), _ptr(grid))
    if rc != 0:
        raise HmsgError(f"hmsg_nav_grid failed ({rc}) (the message is on stderr)")
    return mn, mx, (int(grid[0]), int(grid[1]))


def _nav_call(H, W, top_down, call, device=None):
    """allocates the maps (numpy, or torch tensors on `device`), runs call(out) and repeats it once when the boundary list was too
    short"""
    if device is not None:
        import torch
        buf = lambda shape, np_dtype: torch.empty(shape, dtype=getattr(torch, np.dtype(np_dtype).name), device=device)
    else:
        buf = lambda shape, np_dtype: np.empty(shape, np_dtype)
    maps = dict(obstacle_map=buf((H, W), np.float32), region_map=buf((H, W), np.uint8), poses_map=buf((H, W), np.uint8),
                free_map=buf((H, W), np.uint8), main_free_map=buf((H, W), np.uint8))
    if top_down:
        maps["top_down_bgr"] = buf((H, W, 3), np.uint8)
    cap = 2 * (H + W) + 4096
    out = HmsgNavMaps()
    for attempt in range(2):
        rc_buf = buf((max(cap, 1), 2), np.int32)
        for k, v in maps.items():
            setattr(out, k, _ptr(v))
        out.boundary_rc, out.boundary_capacity = _ptr(rc_buf), cap
        try:
            call(out)
            break
        except HmsgError:
            if attempt == 0 and out.n_boundary > cap:
                cap = int(out.n_boundary)
                continue
            raise
    assert (int(out.grid[0]), int(out.grid[1])) == (W, H)
    maps.update(boundary_rc=rc_buf[: out.n_boundary], n_regions=int(out.n_regions), main_label=int(out.main_label),
                main_area=int(out.main_area), grid=(W, H), pcd_min=np.array(out.pcd_min[:]), pcd_max=np.array(out.pcd_max[:]))
    return maps


def nav_floor_maps(points, colors, zero_level, poses, params=None, device_id=0, lib_: "HmsgLib | None" = None, **over):
    """The navigation maps of a storey on the device (include/hmsg.h: hmsg_nav_floor_maps).  points float64 [n, 3]; colors float64
    [n, 3] in [0, 1] or None (no top-down image); poses [m, 4, 4].  numpy in: numpy out; device tensors in: the maps are device
    tensors and nothing of the storey crosses to the host.  -> dict(obstacle_map f32 [H, W] (NavigationGraph.map), region_map,
    poses_map, free_map, main_free_map u8 [H, W], top_down_bgr u8 [H, W, 3], boundary_rc i32 [k, 2] in row-major order,
    n_regions, main_label, main_area, grid (columns, rows), pcd_min, pcd_max).  params: an HmsgNavParams, or fields by keyword."""
    L = lib_ or lib()
    prm = params if params is not None else nav_params(L, **over)
    on_dev = hasattr(points, "data_ptr") and getattr(points, "is_cuda", False)
    if on_dev:
        import torch
        assert points.dtype == torch.float64 and (colors is None or (colors.dtype == torch.float64 and colors.device == points.device))
        points, colors = points.contiguous(), None if colors is None else colors.contiguous()
        device_id = points.device.index or 0
    else:
        points = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
        colors = None if colors is None else np.ascontiguousarray(np.asarray(colors, np.float64).reshape(-1, 3))
    n = int(points.shape[0])
    assert colors is None or int(colors.shape[0]) == n
    _, _, (W, H) = nav_grid(points, prm.cell_size, device_id, L)
    P_ = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))

    def call(out):
        rc = L.c.hmsg_nav_floor_maps(int(device_id), C.byref(prm), n, _ptr(points), _ptr(colors), float(zero_level), len(P_),
                                     _ptr(P_) if len(P_) else None, C.byref(out))
        if rc != 0:
            raise HmsgError(f"hmsg_nav_floor_maps failed ({rc}) (the message is on stderr)")
    return _nav_call(H, W, colors is not None, call, device=points.device if on_dev else None)


# ---- N7: routes on a floor's free map (include/hmsg.h states the rules R1 to R6)
NAV_UNREACHED = 2147483647


def route_params(lib_: "HmsgLib | None" = None, **over):
    """hmsg_route_params with the defaults (w_straight 5, w_diag 7, min_clearance 0), fields overridden by keyword"""
    L = lib_ or lib()
    p = HmsgRouteParams()
    L.c.hmsg_route_default_params(C.byref(p))
    for k, v in over.items():
        if k not in ("w_straight", "w_diag", "min_clearance"):
            raise HmsgError(f"unknown hmsg_route_params field {k}")
        setattr(p, k, int(v))
    return p


def _is_dev(a):
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)


def _nav_image(a, np_dtype):
    """a [rows, cols] image for the C ABI: a contiguous numpy array, or the device tensor as it is -> (array, rows, cols, device)"""
    if _is_dev(a):
        import torch
        assert a.dtype == getattr(torch, np.dtype(np_dtype).name) and a.dim() == 2, "a device image must have the ABI's dtype"
        return a.contiguous(), int(a.shape[0]), int(a.shape[1]), a.device
    a = np.ascontiguousarray(np.asarray(a, np_dtype))
    assert a.ndim == 2
    return a, int(a.shape[0]), int(a.shape[1]), None


def _nav_cells(a):
    """(row, col) pairs for the C ABI: int32 [n, 2], numpy or a device tensor"""
    if _is_dev(a):
        import torch
        assert a.dtype == torch.int32
        return a.reshape(-1, 2).contiguous()
    a = np.asarray(a)
    return np.ascontiguousarray(a.astype(np.int32).reshape(-1, 2)) if a.dtype != np.int32 else np.ascontiguousarray(a.reshape(-1, 2))


def _nav_buf(device):
    if device is not None:
        import torch
        return lambda shape, np_dtype: torch.empty(shape, dtype=getattr(torch, np.dtype(np_dtype).name), device=device)
    return lambda shape, np_dtype: np.empty(shape, np_dtype)


def _nav_dev_id(device, device_id):
    return (device.index or 0) if device is not None else int(device_id)


def _nav_ck(rc, fn):
    if rc != 0:
        raise HmsgError(f"{fn} failed ({rc}) (the message is on stderr)")


def nav_clearance(mask, params=None, device_id=0, lib_: "HmsgLib | None" = None, **over):
    """R3: the clearance of a mask u8 [rows, cols] (numpy in: numpy out; a device tensor in: a device tensor out) -> int32 [rows, cols]"""
    L = lib_ or lib()
    prm = params if params is not None else route_params(L, **over)
    mask, H, W, dev = _nav_image(mask, np.uint8)
    out = _nav_buf(dev)((H, W), np.int32)
    _nav_ck(L.c.hmsg_nav_clearance(_nav_dev_id(dev, device_id), H, W, _ptr(mask), C.byref(prm), _ptr(out)), "hmsg_nav_clearance")
    return out


def nav_distance_fields(passable, source_sets, params=None, device_id=0, lib_: "HmsgLib | None" = None, **over):
    """R2: one field per source set.  passable u8 [rows, cols]; source_sets: a list of (row, col) arrays [k, 2], or the pair
    (src_off int64 [n + 1], src_rc int32 [m, 2]) -> (fields int32 [n, rows, cols], n_reached int64 [n])"""
    L = lib_ or lib()
    prm = params if params is not None else route_params(L, **over)
    passable, H, W, dev = _nav_image(passable, np.uint8)
    if isinstance(source_sets, tuple) and len(source_sets) == 2 and np.ndim(source_sets[0]) == 1:
        off, rc = np.ascontiguousarray(np.asarray(source_sets[0], np.int64)), _nav_cells(source_sets[1])
    else:
        sets = [np.asarray(s_, np.int64).reshape(-1, 2) for s_ in source_sets]
        off = np.concatenate([[0], np.cumsum([len(s_) for s_ in sets])]).astype(np.int64)
        rc = _nav_cells(np.concatenate(sets) if sets else np.zeros((0, 2)))
    n = len(off) - 1
    buf = _nav_buf(dev)
    fields, reached = buf((n, H, W), np.int32), buf((n,), np.int64)
    _nav_ck(L.c.hmsg_nav_distance_fields(_nav_dev_id(dev, device_id), H, W, _ptr(passable), C.byref(prm), n, _ptr(off),
                                         _ptr(rc) if len(rc) else None, _ptr(fields), _ptr(reached)), "hmsg_nav_distance_fields")
    return fields, reached


def nav_snap_cells(passable, targets_rc, field=None, device_id=0, lib_: "HmsgLib | None" = None):
    """R4: the nearest candidate cell of every target -> (snapped int32 [n, 2], d2 int64 [n]); field: only reached cells are candidates"""
    L = lib_ or lib()
    passable, H, W, dev = _nav_image(passable, np.uint8)
    if field is not None:
        field, fh, fw, fdev = _nav_image(field, np.int32)
        assert (fh, fw) == (H, W) and (fdev is None) == (dev is None)
    t = _nav_cells(targets_rc)
    n = int(t.shape[0])
    buf = _nav_buf(dev)
    snapped, d2 = buf((n, 2), np.int32), buf((n,), np.int64)
    _nav_ck(L.c.hmsg_nav_snap_cells(_nav_dev_id(dev, device_id), H, W, _ptr(passable), _ptr(field), n, _ptr(t) if n else None,
                                    _ptr(snapped) if n else None, _ptr(d2) if n else None), "hmsg_nav_snap_cells")
    return snapped, d2


def nav_paths(passable, field, goals_rc, params=None, device_id=0, lib_: "HmsgLib | None" = None, **over):
    """R5: the cells of the way from the field's source to every goal -> (path_off int64 [n + 1], path_rc int32 [k, 2]).  The
    first call counts, the second writes."""
    L = lib_ or lib()
    prm = params if params is not None else route_params(L, **over)
    passable, H, W, dev = _nav_image(passable, np.uint8)
    field, fh, fw, fdev = _nav_image(field, np.int32)
    assert (fh, fw) == (H, W) and (fdev is None) == (dev is None)
    g = _nav_cells(goals_rc)
    n = int(g.shape[0])
    buf = _nav_buf(dev)
    off, need = buf((n + 1,), np.int64), C.c_int64(0)
    args = (_nav_dev_id(dev, device_id), H, W, _ptr(passable), C.byref(prm), _ptr(field), n, _ptr(g) if n else None)
    _nav_ck(L.c.hmsg_nav_paths(*args, _ptr(off), None, 0, C.byref(need)), "hmsg_nav_paths")
    rc = buf((max(need.value, 1), 2), np.int32)
    _nav_ck(L.c.hmsg_nav_paths(*args, _ptr(off), _ptr(rc), need.value, C.byref(need)), "hmsg_nav_paths")
    return off, rc[: need.value]


def nav_route(main_free_map, start_rc, goals_rc, params=None, device_id=0, lib_: "HmsgLib | None" = None, want_field=False, **over):
    """hmsg_nav_route: the composition on one map -> dict(start_cell (row, col), start_d2, goal_cell int32 [n, 2], goal_d2 int64 [n],
    goal_dist int32 [n], path_off int64 [n + 1], path_rc int32 [k, 2], passable u8 [rows, cols]; field int32 [rows, cols] with
    want_field).  A device tensor in: device tensors out.  The path list is sized by a first guess and the call repeated once."""
    L = lib_ or lib()
    prm = params if params is not None else route_params(L, **over)
    m, H, W, dev = _nav_image(main_free_map, np.uint8)
    start = np.ascontiguousarray(np.asarray(start_rc, np.int64).reshape(2).astype(np.int32))
    g = _nav_cells(goals_rc)
    n = int(g.shape[0])
    buf = _nav_buf(dev)
    res = dict(goal_cell=buf((n, 2), np.int32), goal_d2=buf((n,), np.int64), goal_dist=buf((n,), np.int32), path_off=buf((n + 1,), np.int64),
               passable=buf((H, W), np.uint8))
    if want_field:
        res["field"] = buf((H, W), np.int32)
    out = HmsgNavRoutes()
    cap = max(1, n) * 2 * (H + W)
    for attempt in range(2):
        rc = buf((max(cap, 1), 2), np.int32)
        for k, v in res.items():
            setattr(out, k, _ptr(v))
        out.path_rc, out.path_capacity = _ptr(rc), cap
        status = L.c.hmsg_nav_route(_nav_dev_id(dev, device_id), H, W, _ptr(m), C.byref(prm), _ptr(start), n, _ptr(g) if n else None, C.byref(out))
        if status != 0 and attempt == 0 and out.n_path_cells > cap:
            cap = int(out.n_path_cells)
            continue
        _nav_ck(status, "hmsg_nav_route")
        break
    res.update(path_rc=rc[: out.n_path_cells], start_cell=(int(out.start_cell[0]), int(out.start_cell[1])), start_d2=int(out.start_d2))
    return res


# ---- N8: viewpoints on a floor's free map (include/hmsg.h states the rules V1 to V5)
def view_params(lib_: "HmsgLib | None" = None, **over):
    """hmsg_view_params with the defaults (r_min2 0, r_max2 100 * 100, prefer 0), fields overridden by keyword"""
    L = lib_ or lib()
    p = HmsgViewParams()
    L.c.hmsg_view_default_params(C.byref(p))
    for k, v in over.items():
        if k not in ("r_min2", "r_max2", "prefer"):
            raise HmsgError(f"unknown hmsg_view_params field {k}")
        setattr(p, k, int(v))
    return p


def nav_viewpoints(blocking, passable, goals_rc, field=None, params=None, want_visible=False, device_id=0, lib_: "HmsgLib | None" = None,
                   **over):
    """V3 / V4: the viewpoint of every goal -> dict(view_rc int32 [n, 2], view_d2 int64 [n], view_dist int32 [n], n_visible int32
    [n]; visible u8 [n, rows, cols] with want_visible).  blocking, passable u8 [rows, cols]; field int32 [rows, cols] or None.
    numpy in: numpy out; device tensors in: device tensors out."""
    L = lib_ or lib()
    prm = params if params is not None else view_params(L, **over)
    blocking, H, W, dev = _nav_image(blocking, np.uint8)
    passable, ph, pw, pdev = _nav_image(passable, np.uint8)
    assert (ph, pw) == (H, W) and (pdev is None) == (dev is None)
    if field is not None:
        field, fh, fw, fdev = _nav_image(field, np.int32)
        assert (fh, fw) == (H, W) and (fdev is None) == (dev is None)
    g = _nav_cells(goals_rc)
    n = int(g.shape[0])
    buf = _nav_buf(dev)
    res = dict(view_rc=buf((n, 2), np.int32), view_d2=buf((n,), np.int64), view_dist=buf((n,), np.int32), n_visible=buf((n,), np.int32))
    if want_visible:
        res["visible"] = buf((n, H, W), np.uint8)
    some = lambda a: _ptr(a) if n else None
    _nav_ck(L.c.hmsg_nav_viewpoints(_nav_dev_id(dev, device_id), H, W, _ptr(blocking), _ptr(passable), _ptr(field), C.byref(prm), n, some(g),
                                    some(res["view_rc"]), some(res["view_d2"]), some(res["view_dist"]), some(res["n_visible"]),
                                    some(res["visible"]) if want_visible else None), "hmsg_nav_viewpoints")
    return res


def nav_view_route(main_free_map, blocking, start_rc, goals_rc, params=None, view=None, device_id=0, lib_: "HmsgLib | None" = None,
                   want_field=False, **over):
    """hmsg_nav_view_route: nav_route with the goals' cells chosen by V4 (in sight of the goal on `blocking`) in R4's place -> nav_route's
    dict plus n_visible int32 [n].  Keywords: the fields of hmsg_route_params and of hmsg_view_params."""
    L = lib_ or lib()
    vkeys = ("r_min2", "r_max2", "prefer")
    prm = params if params is not None else route_params(L, **{k: v for k, v in over.items() if k not in vkeys})
    vprm = view if view is not None else view_params(L, **{k: v for k, v in over.items() if k in vkeys})
    m, H, W, dev = _nav_image(main_free_map, np.uint8)
    blocking, bh, bw, bdev = _nav_image(blocking, np.uint8)
    assert (bh, bw) == (H, W) and (bdev is None) == (dev is None)
    start = np.ascontiguousarray(np.asarray(start_rc, np.int64).reshape(2).astype(np.int32))
    g = _nav_cells(goals_rc)
    n = int(g.shape[0])
    buf = _nav_buf(dev)
    res = dict(goal_cell=buf((n, 2), np.int32), goal_d2=buf((n,), np.int64), goal_dist=buf((n,), np.int32), path_off=buf((n + 1,), np.int64),
               passable=buf((H, W), np.uint8))
    if want_field:
        res["field"] = buf((H, W), np.int32)
    n_visible = buf((n,), np.int32)
    out = HmsgNavRoutes()
    cap = max(1, n) * 2 * (H + W)
    for attempt in range(2):
        rc = buf((max(cap, 1), 2), np.int32)
        for k, v in res.items():
            setattr(out, k, _ptr(v))
        out.path_rc, out.path_capacity = _ptr(rc), cap
        status = L.c.hmsg_nav_view_route(_nav_dev_id(dev, device_id), H, W, _ptr(m), _ptr(blocking), C.byref(prm), C.byref(vprm), _ptr(start), n,
                                         _ptr(g) if n else None, C.byref(out), _ptr(n_visible) if n else None)
        if status != 0 and attempt == 0 and out.n_path_cells > cap:
            cap = int(out.n_path_cells)
            continue
        _nav_ck(status, "hmsg_nav_view_route")
        break
    res.update(path_rc=rc[: out.n_path_cells], start_cell=(int(out.start_cell[0]), int(out.start_cell[1])), start_d2=int(out.start_d2),
               n_visible=n_visible)
    return res


# ---- N10: a storey's height map and sight with heights (include/hmsg.h states the rules H1 to H3 and S1 to S5)
def height_params(lib_: "HmsgLib | None" = None, **over):
    """hmsg_height_params with the defaults (cell_size 0.03, height_unit 0.01, top_max 2.5, dilation 5), fields overridden by keyword"""
    L = lib_ or lib()
    p = HmsgHeightParams()
    L.c.hmsg_height_default_params(C.byref(p))
    for k, v in over.items():
        if k not in ("cell_size", "height_unit", "top_max", "dilation"):
            raise HmsgError(f"unknown hmsg_height_params field {k}")
        setattr(p, k, int(v) if k == "dilation" else float(v))
    return p


def _height_call(H, W, device, call):
    """allocates top and known (numpy, or torch tensors on `device`) and runs call(top, known, pcd_min, pcd_max, grid) on their pointers"""
    buf = _nav_buf(device)
    top, known = buf((H, W), np.uint16), buf((H, W), np.uint8)
    mn, mx, grid = np.zeros(3), np.zeros(3), np.zeros(2, np.int32)
    call(_ptr(top), _ptr(known), _ptr(mn), _ptr(mx), _ptr(grid))
    assert (int(grid[0]), int(grid[1])) == (W, H)
    return dict(top=top, known=known, grid=(W, H), pcd_min=mn, pcd_max=mx)


def nav_height_map(points, zero_level, params=None, device_id=0, lib_: "HmsgLib | None" = None, **over):
    """H1 to H3: the height map of a storey's cloud (hmsg_nav_height_map).  points float64 [n, 3], numpy or a device tensor (then
    the maps are device tensors) -> dict(top u16 [rows, cols] in height units above zero_level, known u8 [rows, cols], grid
    (columns, rows), pcd_min, pcd_max).  params: an HmsgHeightParams, or fields by keyword."""
    L = lib_ or lib()
    prm = params if params is not None else height_params(L, **over)
    on_dev = _is_dev(points)
    if on_dev:
        import torch
        assert points.dtype == torch.float64
        points = points.contiguous()
        device_id = points.device.index or 0
    else:
        points = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    n = int(points.shape[0])
    _, _, (W, H) = nav_grid(points, prm.cell_size, device_id, L)
    return _height_call(H, W, points.device if on_dev else None, lambda top, known, mn, mx, grid: _nav_ck(
        L.c.hmsg_nav_height_map(int(device_id), C.byref(prm), n, _ptr(points), float(zero_level), top, known, mn, mx, grid), "hmsg_nav_height_map"))


def _nav_goal_heights(goal_h, goal_r2, n, dev):
    """goal_h int32 [n] and goal_r2 int64 [n] or None for the C ABI, where the images are (a scalar counts for every goal)"""
    def one(a, np_dtype):
        if _is_dev(a):
            import torch
            assert a.dtype == getattr(torch, np.dtype(np_dtype).name) and a.numel() == n
            return a.reshape(-1).contiguous()
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.int64).clip(np.iinfo(np_dtype).min, np.iinfo(np_dtype).max), (n,)).astype(np_dtype))
        if dev is not None:
            import torch
            return torch.from_numpy(a).to(dev)
        return a
    return one(goal_h, np.int32), None if goal_r2 is None else one(goal_r2, np.int64)


def nav_viewpoints_h(top, passable, goals_rc, eye, goal_h, goal_r2=None, field=None, params=None, want_visible=False, device_id=0,
                     lib_: "HmsgLib | None" = None, **over):
    """S3 / S4: nav_viewpoints with sight judged on the height map `top` u16 [rows, cols] (hmsg_nav_viewpoints_h).  eye: the
    camera's height in height units; goal_h [n] (or one value): the goals' heights; goal_r2 [n], one value or None: their
    footprints (squared radius in cells).  -> nav_viewpoints' dict; numpy in: numpy out, device tensors in: device tensors out."""
    L = lib_ or lib()
    prm = params if params is not None else view_params(L, **over)
    top, H, W, dev = _nav_image(top, np.uint16)
    passable, ph, pw, pdev = _nav_image(passable, np.uint8)
    assert (ph, pw) == (H, W) and (pdev is None) == (dev is None)
    if field is not None:
        field, fh, fw, fdev = _nav_image(field, np.int32)
        assert (fh, fw) == (H, W) and (fdev is None) == (dev is None)
    g = _nav_cells(goals_rc)
    n = int(g.shape[0])
    gh, gr2 = _nav_goal_heights(goal_h, goal_r2, n, dev)
    buf = _nav_buf(dev)
    res = dict(view_rc=buf((n, 2), np.int32), view_d2=buf((n,), np.int64), view_dist=buf((n,), np.int32), n_visible=buf((n,), np.int32))
    if want_visible:
        res["visible"] = buf((n, H, W), np.uint8)
    some = lambda a: _ptr(a) if n and a is not None else None
    _nav_ck(L.c.hmsg_nav_viewpoints_h(_nav_dev_id(dev, device_id), H, W, _ptr(top), _ptr(passable), _ptr(field), C.byref(prm), int(eye), n, some(g),
                                      some(gh), some(gr2), some(res["view_rc"]), some(res["view_d2"]), some(res["view_dist"]),
                                      some(res["n_visible"]), some(res["visible"]) if want_visible else None), "hmsg_nav_viewpoints_h")
    return res


def nav_view_route_h(main_free_map, top, start_rc, goals_rc, eye, goal_h, goal_r2=None, params=None, view=None, device_id=0,
                     lib_: "HmsgLib | None" = None, want_field=False, **over):
    """hmsg_nav_view_route_h: nav_view_route with sight judged on the height map `top` (S3 in V3's place) -> nav_view_route's dict"""
    L = lib_ or lib()
    vkeys = ("r_min2", "r_max2", "prefer")
    prm = params if params is not None else route_params(L, **{k: v for k, v in over.items() if k not in vkeys})
    vprm = view if view is not None else view_params(L, **{k: v for k, v in over.items() if k in vkeys})
    m, H, W, dev = _nav_image(main_free_map, np.uint8)
    top, th, tw, tdev = _nav_image(top, np.uint16)
    assert (th, tw) == (H, W) and (tdev is None) == (dev is None)
    start = np.ascontiguousarray(np.asarray(start_rc, np.int64).reshape(2).astype(np.int32))
    g = _nav_cells(goals_rc)
    n = int(g.shape[0])
    gh, gr2 = _nav_goal_heights(goal_h, goal_r2, n, dev)
    buf = _nav_buf(dev)
    res = dict(goal_cell=buf((n, 2), np.int32), goal_d2=buf((n,), np.int64), goal_dist=buf((n,), np.int32), path_off=buf((n + 1,), np.int64),
               passable=buf((H, W), np.uint8))
    if want_field:
        res["field"] = buf((H, W), np.int32)
    n_visible = buf((n,), np.int32)
    out = HmsgNavRoutes()
    cap = max(1, n) * 2 * (H + W)
    some = lambda a: _ptr(a) if n and a is not None else None
    for attempt in range(2):
        rc = buf((max(cap, 1), 2), np.int32)
        for k, v in res.items():
            setattr(out, k, _ptr(v))
        out.path_rc, out.path_capacity = _ptr(rc), cap
        status = L.c.hmsg_nav_view_route_h(_nav_dev_id(dev, device_id), H, W, _ptr(m), _ptr(top), C.byref(prm), C.byref(vprm), int(eye), _ptr(start),
                                           n, some(g), some(gh), some(gr2), C.byref(out), some(n_visible))
        if status != 0 and attempt == 0 and out.n_path_cells > cap:
            cap = int(out.n_path_cells)
            continue
        _nav_ck(status, "hmsg_nav_view_route_h")
        break
    res.update(path_rc=rc[: out.n_path_cells], start_cell=(int(out.start_cell[0]), int(out.start_cell[1])), start_d2=int(out.start_d2),
               n_visible=n_visible)
    return res


# ---- N9: routes across storeys (include/hmsg.h states the rules B1 to B6)
def nav_seeded_fields(passable, seed_sets, params=None, device_id=0, lib_: "HmsgLib | None" = None, **over):
    """B1: one field per seed set.  passable u8 [rows, cols]; seed_sets: a list of (cells [k, 2], costs [k]) pairs, or the triple
    (seed_off int64 [n + 1], seed_rc int32 [m, 2], seed_cost int32 [m]) -> (fields int32 [n, rows, cols], n_reached int64 [n])"""
    L = lib_ or lib()
    prm = params if params is not None else route_params(L, **over)
    passable, H, W, dev = _nav_image(passable, np.uint8)
    if isinstance(seed_sets, tuple) and len(seed_sets) == 3 and np.ndim(seed_sets[0]) == 1:
        off, rc = np.ascontiguousarray(np.asarray(seed_sets[0], np.int64)), _nav_cells(seed_sets[1])
        cost = np.ascontiguousarray(np.asarray(seed_sets[2], np.int64).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32).reshape(-1))
    else:
        cells = [np.asarray(c_, np.int64).reshape(-1, 2) for c_, _ in seed_sets]
        costs = [np.asarray(v_, np.int64).reshape(-1) for _, v_ in seed_sets]
        assert all(len(c_) == len(v_) for c_, v_ in zip(cells, costs)), "a cost per seed"
        off = np.concatenate([[0], np.cumsum([len(c_) for c_ in cells])]).astype(np.int64)
        rc = _nav_cells(np.concatenate(cells) if cells else np.zeros((0, 2)))
        cost = np.ascontiguousarray((np.concatenate(costs) if costs else np.zeros(0)).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32))
    n = len(off) - 1
    buf = _nav_buf(dev)
    fields, reached = buf((n, H, W), np.int32), buf((n,), np.int64)
    _nav_ck(L.c.hmsg_nav_seeded_fields(_nav_dev_id(dev, device_id), H, W, _ptr(passable), C.byref(prm), n, _ptr(off),
                                       _ptr(rc) if len(rc) else None, _ptr(cost) if len(cost) else None, _ptr(fields), _ptr(reached)),
            "hmsg_nav_seeded_fields")
    return fields, reached


class _NavBuilding:
    """a building for the C ABI: the storeys' images (all numpy or all device tensors), shapes, the array of pointers, the links"""

    def __init__(self, images, links, np_dtype=np.uint8):
        assert len(images) >= 1, "a building has a storey"
        got = [_nav_image(m, np_dtype) for m in images]
        self.images = [g[0] for g in got]
        self.shapes = [(g[1], g[2]) for g in got]
        self.dev = got[0][3]
        assert all((g[3] is None) == (self.dev is None) for g in got), "the storeys' images: all host or all device memory"
        self.n = len(got)
        self.rows = np.array([h for h, _ in self.shapes], np.int32)
        self.cols = np.array([w for _, w in self.shapes], np.int32)
        self.ptrs = self.pointers(self.images)
        ln = np.asarray(links if links is not None and len(links) else np.zeros((0, 7)), np.int64).reshape(-1, 7)
        self.links = np.ascontiguousarray(ln.clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32))

    @staticmethod
    def pointers(arrays):
        return (C.c_void_p * len(arrays))(*[_ptr(a) for a in arrays])

    def head(self, device_id):
        return (_nav_dev_id(self.dev, device_id), self.n, _ptr(self.rows), _ptr(self.cols), self.ptrs, len(self.links),
                _ptr(self.links) if len(self.links) else None)


def _nav_triples(a):
    """(storey, row, col) triples for the C ABI: int32 [n, 3] on the host (the library reads them there)"""
    a = np.asarray(a.cpu() if hasattr(a, "cpu") else a)
    return np.ascontiguousarray(np.asarray(a, np.int64).reshape(-1, 3).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32))


def nav_building_fields(passables, links, starts, params=None, device_id=0, lib_: "HmsgLib | None" = None, **over):
    """B3: the building fields of every start.  passables: a list of u8 [rows_l, cols_l] (numpy, or device tensors: then the fields
    are device tensors); links int [k, 7] (sa, ra, ca, sb, rb, cb, cost); starts int [n, 3] (storey, row, col) -> (fields: a list
    with one int32 [n, rows_l, cols_l] per storey, n_reached int64 [n, storeys])"""
    L = lib_ or lib()
    prm = params if params is not None else route_params(L, **over)
    b = _NavBuilding(passables, links)
    st = _nav_triples(starts)
    n = len(st)
    buf = _nav_buf(b.dev)
    fields = [buf((n, h, w), np.int32) for h, w in b.shapes]
    reached = buf((n, b.n), np.int64)
    _nav_ck(L.c.hmsg_nav_building_fields(*b.head(device_id), C.byref(prm), n, _ptr(st) if n else None, b.pointers(fields), _ptr(reached)),
            "hmsg_nav_building_fields")
    return fields, reached


def nav_building_paths(passables, links, fields, goals, params=None, device_id=0, lib_: "HmsgLib | None" = None, **over):
    """B5 on the building field of one start (fields: one int32 [rows_l, cols_l] per storey) -> (path_off int64 [n + 1], path_src
    int32 [k, 3]: storey, row, col).  The first call counts, the second writes."""
    L = lib_ or lib()
    prm = params if params is not None else route_params(L, **over)
    b = _NavBuilding(passables, links)
    f = _NavBuilding(fields, None, np.int32)
    assert f.shapes == b.shapes and (f.dev is None) == (b.dev is None)
    g = _nav_triples(goals)
    n = len(g)
    buf = _nav_buf(b.dev)
    off, need = buf((n + 1,), np.int64), C.c_int64(0)
    args = b.head(device_id) + (C.byref(prm), f.ptrs, n, _ptr(g) if n else None)
    _nav_ck(L.c.hmsg_nav_building_paths(*args, _ptr(off), None, 0, C.byref(need)), "hmsg_nav_building_paths")
    src = buf((max(need.value, 1), 3), np.int32)
    _nav_ck(L.c.hmsg_nav_building_paths(*args, _ptr(off), _ptr(src), need.value, C.byref(need)), "hmsg_nav_building_paths")
    return off, src[: need.value]


def nav_building_route(main_free_maps, links, start, goals, params=None, device_id=0, lib_: "HmsgLib | None" = None, want_fields=False, **over):
    """hmsg_nav_building_route: the composition over a building -> dict(start_cell (storey, row, col), start_d2, goal_cell int32
    [n, 3], goal_d2 int64 [n], goal_dist int32 [n], path_off int64 [n + 1], path_src int32 [k, 3], passable: a list of u8 [rows_l,
    cols_l]; fields: a list of int32 [rows_l, cols_l] with want_fields).  Device tensors in: device tensors out.  The path list is
    sized by a first guess and the call repeated once."""
    L = lib_ or lib()
    prm = params if params is not None else route_params(L, **over)
    b = _NavBuilding(main_free_maps, links)
    st = _nav_triples(start).reshape(3)
    g = _nav_triples(goals)
    n = len(g)
    buf = _nav_buf(b.dev)
    res = dict(goal_cell=buf((n, 3), np.int32), goal_d2=buf((n,), np.int64), goal_dist=buf((n,), np.int32), path_off=buf((n + 1,), np.int64))
    passable = [buf((h, w), np.uint8) for h, w in b.shapes]
    fields = [buf((h, w), np.int32) for h, w in b.shapes] if want_fields else None
    keep = (b.pointers(passable), b.pointers(fields) if want_fields else None)
    out = HmsgNavBuildingRoutes()
    cap = max(1, n) * 2 * int(b.rows.sum() + b.cols.sum())
    for attempt in range(2):
        src = buf((max(cap, 1), 3), np.int32)
        for k, v in res.items():
            setattr(out, k, _ptr(v))
        out.path_src, out.path_capacity = _ptr(src), cap
        out.passable = C.cast(keep[0], C.POINTER(C.c_void_p))
        if want_fields:
            out.field = C.cast(keep[1], C.POINTER(C.c_void_p))
        status = L.c.hmsg_nav_building_route(*b.head(device_id), C.byref(prm), _ptr(st), n, _ptr(g) if n else None, C.byref(out))
        if status != 0 and attempt == 0 and out.n_path_cells > cap:
            cap = int(out.n_path_cells)
            continue
        _nav_ck(status, "hmsg_nav_building_route")
        break
    res.update(path_src=src[: out.n_path_cells], start_cell=tuple(int(v) for v in out.start_cell), start_d2=int(out.start_d2), passable=passable)
    if want_fields:
        res["fields"] = fields
    return res


# ---- N11: rooms on a floor's free map (include/hmsg.h states the rules G1, G2, D1 to D4, L1)
def _nav_seed_sets(seed_sets):
    """a list of (row, col) arrays, one per room, or the pair (seed_off int64 [n + 1], seed_rc int32 [m, 2]) -> (off, rc)"""
    if isinstance(seed_sets, tuple) and len(seed_sets) == 2 and np.ndim(seed_sets[0]) == 1:
        return np.ascontiguousarray(np.asarray(seed_sets[0], np.int64)), _nav_cells(seed_sets[1])
    sets = [np.asarray(s_, np.int64).reshape(-1, 2) for s_ in seed_sets]
    off = np.concatenate([[0], np.cumsum([len(s_) for s_ in sets])]).astype(np.int64)
    return off, _nav_cells(np.concatenate(sets) if sets else np.zeros((0, 2)))


def nav_room_labels(passable, seed_sets, params=None, want_dist=False, device_id=0, lib_: "HmsgLib | None" = None, **over):
    """G1, G2: the room of every reached cell (hmsg_nav_room_labels).  passable u8 [rows, cols]; seed_sets as _nav_seed_sets takes
    them -> (label int32 [rows, cols], n_cells int64 [n_rooms]) and, with want_dist, dist int32 [rows, cols] as the third.  A
    device tensor in: device tensors out."""
    L = lib_ or lib()
    prm = params if params is not None else route_params(L, **over)
    passable, H, W, dev = _nav_image(passable, np.uint8)
    off, rc = _nav_seed_sets(seed_sets)
    n = len(off) - 1
    buf = _nav_buf(dev)
    label, cells = buf((H, W), np.int32), buf((max(n, 0),), np.int64)
    dist = buf((H, W), np.int32) if want_dist else None
    _nav_ck(L.c.hmsg_nav_room_labels(_nav_dev_id(dev, device_id), H, W, _ptr(passable), C.byref(prm), n, _ptr(off), _ptr(rc) if len(rc) else None,
                                     _ptr(label), _ptr(dist), _ptr(cells) if n > 0 else None), "hmsg_nav_room_labels")
    return (label, cells, dist) if want_dist else (label, cells)


def _nav_door_call(call, fn, buf, H, W, n_rooms, want_other, want_adjacency):
    """the door table of `call(out)`, with lists as long as the image has cells (only what the counts say is written and kept)"""
    res = {}
    if want_other:
        res["other"] = buf((H, W), np.int32)
    if want_adjacency:
        res["adjacency"] = buf((n_rooms, n_rooms), np.int32)
    out = HmsgNavDoorTable()
    cap = H * W                                                           # no more doors or door cells than cells: never too short
    pair, off, rc = buf((cap, 2), np.int32), buf((cap + 1,), np.int64), buf((cap, 2), np.int32)
    for k, v in res.items():
        setattr(out, k, _ptr(v))
    out.door_pair, out.door_off, out.door_rc, out.door_capacity, out.cell_capacity = _ptr(pair), _ptr(off), _ptr(rc), cap, cap
    _nav_ck(call(out), fn)
    nd, nc = int(out.n_doors), int(out.n_door_cells)
    res.update(door_pair=pair[:nd], door_off=off[: nd + 1], door_rc=rc[:nc], n_doors=nd, n_door_cells=nc)
    return res


def nav_doors(passable, label, n_rooms, want_other=True, want_adjacency=True, device_id=0, lib_: "HmsgLib | None" = None):
    """D1 to D4: the doors between the rooms of a label image (hmsg_nav_doors) -> dict(door_pair int32 [n_doors, 2], door_off int64
    [n_doors + 1], door_rc int32 [n_door_cells, 2], n_doors, n_door_cells; other int32 [rows, cols]; adjacency int32 [n_rooms,
    n_rooms])"""
    L = lib_ or lib()
    passable, H, W, dev = _nav_image(passable, np.uint8)
    label, lh, lw, ldev = _nav_image(label, np.int32)
    assert (lh, lw) == (H, W) and (ldev is None) == (dev is None)
    n_rooms = int(n_rooms)
    call = lambda out: L.c.hmsg_nav_doors(_nav_dev_id(dev, device_id), H, W, _ptr(passable), _ptr(label), n_rooms, C.byref(out))
    return _nav_door_call(call, "hmsg_nav_doors", _nav_buf(dev), H, W, max(n_rooms, 0), want_other, want_adjacency and 0 <= n_rooms <= 4096)


def nav_path_rooms(label, path_off, path_rc, device_id=0, lib_: "HmsgLib | None" = None):
    """L1: the legs of every path by room (hmsg_nav_path_rooms) -> (leg_off int64 [n_paths + 1], leg_room int32 [k], leg_first int64
    [k]).  The first call counts, the second writes."""
    L = lib_ or lib()
    label, H, W, dev = _nav_image(label, np.int32)
    if not _is_dev(path_off):
        path_off = np.ascontiguousarray(np.asarray(path_off, np.int64))
    rc = _nav_cells(path_rc)
    n = int(path_off.shape[0]) - 1
    buf = _nav_buf(dev)
    off, need = buf((n + 1,), np.int64), C.c_int64(0)
    args = (_nav_dev_id(dev, device_id), H, W, _ptr(label), n, _ptr(path_off), _ptr(rc) if len(rc) else None)
    _nav_ck(L.c.hmsg_nav_path_rooms(*args, _ptr(off), None, None, 0, C.byref(need)), "hmsg_nav_path_rooms")
    room, first = buf((max(need.value, 1),), np.int32), buf((max(need.value, 1),), np.int64)
    _nav_ck(L.c.hmsg_nav_path_rooms(*args, _ptr(off), _ptr(room), _ptr(first), need.value, C.byref(need)), "hmsg_nav_path_rooms")
    return off, room[: need.value], first[: need.value]


def nav_room_doors(main_free_map, seed_sets, params=None, want_other=True, want_adjacency=True, device_id=0, lib_: "HmsgLib | None" = None,
                   **over):
    """hmsg_nav_room_doors: passable as nav_route makes it, the labels, the doors, in one call -> nav_doors' dict plus label int32
    [rows, cols] and passable u8 [rows, cols]"""
    L = lib_ or lib()
    prm = params if params is not None else route_params(L, **over)
    m, H, W, dev = _nav_image(main_free_map, np.uint8)
    off, rc = _nav_seed_sets(seed_sets)
    n = len(off) - 1
    buf = _nav_buf(dev)
    label, passable = buf((H, W), np.int32), buf((H, W), np.uint8)
    call = lambda out: L.c.hmsg_nav_room_doors(_nav_dev_id(dev, device_id), H, W, _ptr(m), C.byref(prm), n, _ptr(off), _ptr(rc) if len(rc) else None,
                                               _ptr(label), _ptr(passable), C.byref(out))
    res = _nav_door_call(call, "hmsg_nav_room_doors", buf, H, W, max(n, 0), want_other, want_adjacency and 0 <= n <= 4096)
    res.update(label=label, passable=passable)
    return res


def _clip_params(L, size, f16, mean, std):
    p = HmsgClipPreprocess()
    L.c.hmsg_clip_default_preprocess(C.byref(p))
    p.size, p.out_f16 = int(size), int(bool(f16))
    if mean is not None:
        p.mean[:] = [float(v) for v in mean]
    if std is not None:
        p.std[:] = [float(v) for v in std]
    return p


def clip_preprocess(images, size=224, f16=False, mean=None, std=None, return_u8=False, device_id=0, lib_: "HmsgLib | None" = None):
    """open_clip's inference `preprocess` -- Resize(size, BICUBIC), CenterCrop(size), ToTensor, Normalize -- on the device, equal
    to it in every bit (include/hmsg.h: hmsg_clip_preprocess_batch; utils/clip_utils.py:72-73, 88-89).  images: uint8 [H, W, 3]
    or [B, H, W, 3], a numpy array or a torch tensor on the device.  Returns [.., 3, size, size] float32 (float16 with f16), of
    the kind that came in; with return_u8 also the resized and centre-cropped bytes [.., size, size, 3]."""
    L = lib_ or lib()
    on_dev = hasattr(images, "data_ptr")
    if on_dev:
        import torch
        assert images.dtype == torch.uint8 and images.is_cuda
        images = images.contiguous()
        device_id = images.device.index or 0
    else:
        images = np.ascontiguousarray(images, dtype=np.uint8)
    single = images.ndim == 3
    shape = tuple(images.shape)
    assert len(shape) in (3, 4) and shape[-1] == 3, "images: [H, W, 3] or [B, H, W, 3]"
    B, (H, W) = (1 if single else shape[0]), shape[-3:-1]
    S = int(size)
    if on_dev:
        out = torch.empty((B, 3, S, S), dtype=torch.float16 if f16 else torch.float32, device=images.device)
        u8 = torch.empty((B, S, S, 3), dtype=torch.uint8, device=images.device) if return_u8 else None
    else:
        out = np.empty((B, 3, S, S), np.float16 if f16 else np.float32)
        u8 = np.empty((B, S, S, 3), np.uint8) if return_u8 else None
    p = _clip_params(L, size, f16, mean, std)
    rc = L.c.hmsg_clip_preprocess_batch(device_id, C.byref(p), B, H, W, _ptr(images), _ptr(out), _ptr(u8), None)
    if rc != 0:
        raise HmsgError(f"hmsg_clip_preprocess_batch failed ({rc})")
    if single:
        out, u8 = out[0], (u8[0] if return_u8 else None)
    return (out, u8) if return_u8 else out


def frame_encoder_inputs(image, masks, bbox_margin=0, size=224, crop_size=512, f16=False, mean=None, std=None, device_id=0,
                         lib_: "HmsgLib | None" = None):
    """The 1 + 2 M encoder inputs of one frame (include/hmsg.h: hmsg_frame_encoder_inputs; sam_clip_feats_extractor.py:147-158):
    row 0 the whole frame, rows 1..M the masked crops, rows M + 1..2 M the plain crops, each through clip_preprocess.  `masks`:
    SAM records as crop_all_bounding_boxs takes them.  Returns a numpy array [1 + 2 M, 3, size, size]."""
    L = lib_ or lib()
    image = np.ascontiguousarray(image, dtype=np.uint8)
    H, W = image.shape[:2]
    M = len(masks)
    bbox = np.ascontiguousarray([m["bbox"] for m in masks], dtype=np.float64).reshape(M, 4)
    segs = np.ascontiguousarray(np.stack([m["segmentation"] for m in masks]).astype(np.uint8)) if M else None
    out = np.empty((1 + 2 * M, 3, int(size), int(size)), np.float16 if f16 else np.float32)
    p = _clip_params(L, size, f16, mean, std)
    rc = L.c.hmsg_frame_encoder_inputs(device_id, C.byref(p), H, W, _ptr(image), M, _ptr(segs), _ptr(bbox) if M else None,
                                       float(bbox_margin), int(crop_size), _ptr(out), None)
    if rc != 0:
        raise HmsgError(f"hmsg_frame_encoder_inputs failed ({rc})")
    return out


class NodeIndex:
    """Resident node-embedding table for retrieval (graph.py:3056-3162)."""

    def __init__(self, emb: np.ndarray, room_of_node: np.ndarray, device_id=0, lib_: HmsgLib | None = None):
        self.L = lib_ or lib()
        emb = np.ascontiguousarray(emb)
        assert emb.dtype in (np.float32, np.float64)
        room_of_node = np.ascontiguousarray(room_of_node, dtype=np.int32)
        self.N, self.D = emb.shape
        ix = _P()
        rc = self.L.c.hmsg_index_create(device_id, self.D, self.N, _ptr(emb), int(emb.dtype == np.float64),
                                        _ptr(room_of_node), C.byref(ix))
        if rc != 0:
            raise HmsgError(f"hmsg_index_create failed ({rc})")
        self.ix = ix

    @classmethod
    def load_objects(cls, directory, stems, room_of_node, device_id=0, n_threads=0, lib_: "HmsgLib | None" = None):
        """The object table of a saved graph (objects/<stem>.json, "embedding" arrays as float64) straight into a resident
        index (include/hmsg.h: hmsg_index_load_objects)."""
        L = lib_ or lib()
        n = len(stems)
        arr = (C.c_char_p * max(n, 1))(*[str(s_).encode() for s_ in stems])
        rooms = np.ascontiguousarray(room_of_node, dtype=np.int32)
        ix, d = _P(), C.c_int32(0)
        rc = L.c.hmsg_index_load_objects(device_id, str(directory).encode(), n, C.cast(arr, _P), _ptr(rooms), int(n_threads),
                                         C.byref(ix), C.byref(d))
        if rc != 0:
            raise HmsgError(f"hmsg_index_load_objects failed ({rc})")
        return cls._wrap(L, ix, n, int(d.value))

    @classmethod
    def _wrap(cls, L, ix, n, d):
        self = cls.__new__(cls)
        self.L, self.ix, self.N, self.D = L, ix, n, d
        return self

    def close(self):
        if getattr(self, "ix", None):
            self.L.c.hmsg_index_destroy(self.ix)
            self.ix = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise HmsgError(f"[{rc}] " + self.L.c.hmsg_index_last_error(self.ix).decode())

    def set_profiling(self, on=True):
        self._ck(self.L.c.hmsg_index_set_profiling(self.ix, int(on)))

    def profile(self):
        """(launches, total ms, total FLOP) of the float64 MFMA similarity GEMM."""
        n, ms, fl = C.c_int64(), C.c_double(), C.c_double()
        self._ck(self.L.c.hmsg_index_profile(self.ix, C.byref(n), C.byref(ms), C.byref(fl)))
        return int(n.value), float(ms.value), float(fl.value)

    def set_hierarchy(self, floor_rooms, room_name_emb, room_view_embs, room_keys):
        """floor_rooms: per floor the room ids in floors[f].rooms order; room_name_emb f64 [R, D] (or None);
        room_view_embs: per room an [n_v, D] array (room.embeddings); room_keys: per room int(room_id.split("_")[-1])."""
        R = len(room_view_embs)
        foff = np.zeros(len(floor_rooms) + 1, np.int32)
        foff[1:] = np.cumsum([len(r) for r in floor_rooms])
        fr = np.ascontiguousarray(np.concatenate([np.asarray(r, np.int32) for r in floor_rooms]) if foff[-1] else np.zeros(0, np.int32), np.int32)
        voff = np.zeros(R + 1, np.int64)
        voff[1:] = np.cumsum([len(v) for v in room_view_embs])
        views = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64).reshape(-1, self.D) for v in room_view_embs])
                                     if voff[-1] else np.zeros((0, self.D)), np.float64)
        names = None if room_name_emb is None else np.ascontiguousarray(room_name_emb, np.float64)
        keys = np.ascontiguousarray(room_keys, np.int32)
        self._ck(self.L.c.hmsg_index_set_hierarchy(self.ix, R, len(floor_rooms), _ptr(foff), _ptr(fr), _ptr(names), _ptr(voff),
                                                   _ptr(views), _ptr(keys)))
        self._n_rooms = R

    def query_hier(self, T_obj, qid, T_room, floor_id, room_mode, k, use_negatives=True, max_rooms=None):
        """floor -> room(s) -> objects on the device (include/hmsg.h: hmsg_query_hier).  Returns (rooms per query as
        query_hmsg_room reports them, idx [Q, k], room [Q, k] (global ids), score [Q, k])."""
        # (text rows: numpy arrays, or float32 torch tensors -- on the device they are used where they are: hmsg.h, "host or device pointers")
        if not hasattr(T_obj, "data_ptr"):
            T_obj = np.ascontiguousarray(T_obj, dtype=np.float32)
        Q, Cn, D = T_obj.shape
        if T_room is not None and not hasattr(T_room, "data_ptr"):
            T_room = np.ascontiguousarray(T_room, dtype=np.float32)
        qid = np.ascontiguousarray(qid, dtype=np.int32)
        floor_id = np.ascontiguousarray(floor_id, dtype=np.int32)
        room_mode = np.ascontiguousarray(room_mode, dtype=np.int32)
        RM = int(max_rooms or max(self._n_rooms, 10))
        sel = np.empty((Q, RM), np.int32)
        nsel = np.empty((Q,), np.int32)
        idx = np.empty((Q, k), np.int32)
        room = np.empty((Q, k), np.int32)
        score = np.empty((Q, k), np.float64)
        self._ck(self.L.c.hmsg_query_hier(self.ix, Q, Cn, _ptr(T_obj), _ptr(qid), _ptr(T_room), _ptr(floor_id), _ptr(room_mode), k,
                                          int(use_negatives), RM, _ptr(sel), _ptr(nsel), _ptr(idx), _ptr(room), _ptr(score)))
        return [sel[q, : nsel[q]].tolist() for q in range(Q)], idx, room, score

    def query_objects(self, T, qid, room_lists, k, use_negatives=True):
        T = np.ascontiguousarray(T, dtype=np.float32)
        Q, Cn, D = T.shape
        qid = np.ascontiguousarray(qid, dtype=np.int32)
        off = np.zeros(Q + 1, np.int32)
        off[1:] = np.cumsum([len(r) for r in room_lists])
        rooms = np.ascontiguousarray(np.concatenate([np.asarray(r, np.int32) for r in room_lists]) if off[-1] else
                                     np.zeros(0, np.int32), dtype=np.int32)
        idx = np.empty((Q, k), np.int32)
        room = np.empty((Q, k), np.int32)
        score = np.empty((Q, k), np.float64)
        self._ck(self.L.c.hmsg_query_objects(self.ix, Q, Cn, _ptr(T), _ptr(qid), _ptr(off), _ptr(rooms), k,
                                             int(use_negatives), _ptr(idx), _ptr(room), _ptr(score)))
        return idx, room, score

    def set_views(self, view_lists):
        """hmsg_index_set_views: per view the node indices of its objects, in view.object_ids order"""
        off = np.zeros(len(view_lists) + 1, np.int64)
        for i, l in enumerate(view_lists):
            off[i + 1] = off[i] + len(l)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(l, np.int32).reshape(-1) for l in view_lists]) if len(view_lists) else np.zeros(0), dtype=np.int32)
        if not len(flat):
            flat = np.zeros(1, np.int32)
        self._ck(self.L.c.hmsg_index_set_views(self.ix, len(view_lists), _ptr(off), _ptr(flat)))

    def rematch_in_views(self, T, view):
        """hmsg_rematch_in_views -> (node [Q] (-1: a view without objects), score [Q])"""
        T = np.ascontiguousarray(T, dtype=np.float32)
        view = np.ascontiguousarray(view, dtype=np.int32)
        node, score = np.empty(len(T), np.int32), np.empty(len(T), np.float64)
        self._ck(self.L.c.hmsg_rematch_in_views(self.ix, len(T), _ptr(T), _ptr(view), _ptr(node), _ptr(score)))
        return node, score

    def similarity(self, T):
        T = np.ascontiguousarray(T, dtype=np.float32)
        S = np.empty((T.shape[0], self.N), np.float64)
        self._ck(self.L.c.hmsg_similarity(self.ix, T.shape[0], _ptr(T), _ptr(S)))
        return S
