// The view level of the slow path (hmsg_query_views.hip) as the graph object (hmsg_scene_graph.hip) drives it: the resident table
// of sampled-image embeddings with its exact top-k, and the cloud-in-view distances over clouds that are already in HBM.
#pragma once
#include "hmsg_common.h"

#include <vector>

// ---- goal views: every sampled image of every room, float64 in HBM, rows in self.rooms order and within a room in sample_images order
struct hmsg_goal_table;
// img_off [n_rooms + 1] (rows of room r), clip f32 [rows][D], img_id [rows]; floors -> rooms as hmsg_index_set_hierarchy takes them
hmsg_goal_table* hmsg_goal_table_create(int device, int D, int n_rooms, const std::vector<int>& img_off, const std::vector<float>& clip,
                                        const std::vector<long long>& img_id, const std::vector<int>& floor_room_off, const std::vector<int>& floor_rooms);
void hmsg_goal_table_free(hmsg_goal_table* t);
// Q text rows T f32 [Q][D] (host or device), floor_id [Q] (host; -1: every room) -> per query the k best rows of its rooms list:
// descending score, exact ties by ascending candidate position (room place in the list, then image place in the room).  Outputs
// host or device, -1 / 0.0 past out_n[q].  Throws hmsg_error.
void hmsg_goal_table_topk(hmsg_goal_table* t, int Q, const float* T, const int* floor_id, int k, long long* out_img, int* out_room, double* out_score,
                          int* out_n);

// ---- cloud-in-view distances: pair p = the points of segs[seg_off[p] .. seg_off[p + 1]) of d_pts (device, f64 [.][3]) one after the
// other, seen through pose_inv [p][16] (world -> camera), K [9], wh [p][2] (host arrays).  Host outputs, each optional:
//   avg_z_front  mean camera z of the points with z > 0, NaN without one      (visualize_pcd_on_image, utils/graph_utils.py:49-70)
//   visible, mean_depth  as hmsg_object_views defines them                    (check_object_in_view, utils/graph_utils.py:95-157)
struct CloudSeg {
    long long p0, n;
};
void hmsg_view_depths(hipStream_t s, const double* d_pts, long long n_pairs, const std::vector<long long>& seg_off, const std::vector<CloudSeg>& segs,
                      const double* pose_inv, const int* wh, const double* K, double min_visible_ratio, double max_depth, double* avg_z_front,
                      unsigned char* visible, double* mean_depth);
