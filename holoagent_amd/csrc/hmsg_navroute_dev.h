// What hmsg_navview.hip (N8) shares with hmsg_navroute.hip (N7): R4's snap on device buffers, and the body of hmsg_nav_route with
// the step that chooses the goals' cells handed in, so that hmsg_nav_view_route is that body with V4 in R4's place and only that.
#pragma once
#include "hmsg_boundary.h"

#include <functional>

// the cells of the goals (d_goal, i32 [n][2]) among the reached cells of d_field on d_pass: d_cell i32 [n][2], (-1, -1) for none;
// d_d2 i64 [n] or nullptr.  All device memory, all work on s.
using navr_goal_snap =
    std::function<void(hipStream_t s, const unsigned char* d_pass, const int* d_field, const int* d_goal, int* d_cell, long long* d_d2)>;

void navr_snap_dev(hipStream_t s, int rows, int cols, const unsigned char* d_pass, const int* d_field, long long n, const int* d_target,
                   int* d_snapped, long long* d_d2);
// fn: the entry point's name for the messages.  Checks the shape and prm as hmsg_nav_route does; ends in a stream synchronise.
void navr_route_run(const char* fn, int32_t rows, int32_t cols, const uint8_t* main_free_map, const hmsg_route_params* prm, const int32_t* start_rc,
                    int64_t n_goals, const int32_t* goal_rc, hmsg_nav_routes* out, const navr_goal_snap& snap);
