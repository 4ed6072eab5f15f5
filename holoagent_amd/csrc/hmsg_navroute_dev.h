// What hmsg_navview.hip (N8) shares with hmsg_navroute.hip (N7): R4's snap on device buffers, and the body of hmsg_nav_route with
// the step that chooses the goals' cells handed in, so that hmsg_nav_view_route is that body with V4 in R4's place and only that.
#pragma once
#include "hmsg_boundary.h"

#include <functional>

#define NAVR_T 256                       // threads of a workgroup of the routing kernels
#define NAVR_TILE 64                     // the side of a tile of the relaxation: a stamp in `act` speaks of one tile
#define NAVR_SIDE (NAVR_TILE + 2)        // ... with its one-cell halo
#define NAVR_LD 67                       // LDS row stride of a tile of int32 in words (odd: 64 lanes of a sweep hit 64 banks)
#define NAVR_PLD 68                      // ... and of the passable bytes

// the cells of the goals (d_goal, i32 [n][2]) among the reached cells of d_field on d_pass: d_cell i32 [n][2], (-1, -1) for none;
// d_d2 i64 [n] or nullptr.  All device memory, all work on s.
using navr_goal_snap =
    std::function<void(hipStream_t s, const unsigned char* d_pass, const int* d_field, const int* d_goal, int* d_cell, long long* d_d2)>;

void navr_snap_dev(hipStream_t s, int rows, int cols, const unsigned char* d_pass, const int* d_field, long long n, const int* d_target,
                   int* d_snapped, long long* d_d2);
// fn: the entry point's name for the messages.  Checks the shape and prm as hmsg_nav_route does; ends in a stream synchronise.
void navr_route_run(const char* fn, int32_t rows, int32_t cols, const uint8_t* main_free_map, const hmsg_route_params* prm, const int32_t* start_rc,
                    int64_t n_goals, const int32_t* goal_rc, hmsg_nav_routes* out, const navr_goal_snap& snap);

// What hmsg_navbuilding.hip (N9) shares with hmsg_navroute.hip: the relaxation itself.  navr_relax_round enqueues ONE round over
// all tiles of the nf fields d_field i32 [nf][rows][cols] (a tile runs when its stamp in d_act i32 [nf][tiles] is >= round, a tile
// that changed stamps its eight neighbours round + 1 and adds 1 to *d_changed); navr_relax enqueues rounds in growing batches until
// the last round of a batch changed no tile, and counts rounds and host round trips for hmsg_test_nav_route_last
// (navr_last_reset zeroes the two).  corner: R1's rule for diagonal moves; d_pass == nullptr: every cell passable.
void navr_check(int32_t rows, int32_t cols, const hmsg_route_params& p, const char* fn);
void navr_last_reset();
void navr_relax_round(hipStream_t s, int rows, int cols, const unsigned char* d_pass, const hmsg_route_params& p, bool corner, int nf, int* d_field,
                      int* d_act, int round, unsigned* d_changed);
void navr_relax(hipStream_t s, int rows, int cols, const unsigned char* d_pass, const hmsg_route_params& p, bool corner, int nf, int* d_field,
                int* d_act);
// d_pass = the mask where its clearance reaches p.min_clearance (0: the mask as 1 / 0): hmsg_nav_route's first step
void navr_passable_dev(hipStream_t s, int rows, int cols, const unsigned char* d_mask, const hmsg_route_params& p, unsigned char* d_pass);
void navr_fill_dev(hipStream_t s, int* d_p, long long n, int v);
// one wave: d_off [n + 1] = the exclusive scan of d_cnt [n] and the sum
void navr_scan_dev(hipStream_t s, long long n, const long long* d_cnt, long long* d_off);
[[noreturn]] void navr_throw_short(const char* fn, long long total, long long capacity);

// What hmsg_navrooms.hip (N11) shares with hmsg_navroute.hip: the fields themselves and the loop of rounds.  navr_fields_dev makes
// d_fields i32 [nf][rows][cols] from the sources d_src_rc[d_src_off[f] .. d_src_off[f + 1]) (device memory; max_sources: the most
// of one field; d_n_reached u64 [nf] or nullptr).  navr_rounds calls enqueue(round, d_changed) for round 1, 2, ... in batches of 4,
// 8, 16, then 32 rounds, reads the batch's counters back once and ends when the last round of a batch left its counter 0; it counts
// rounds and round trips as navr_relax does (which is navr_rounds over navr_relax_round).  navr_last_get reads the two counts.
using navr_round_fn = std::function<void(int round, unsigned* d_changed)>;
void navr_rounds(hipStream_t s, const navr_round_fn& enqueue);
void navr_last_get(int* rounds, int* trips);
void navr_fields_dev(hipStream_t s, int rows, int cols, const unsigned char* d_pass, const hmsg_route_params& p, long long nf_all,
                     const long long* d_src_off, const int* d_src_rc, long long max_sources, int* d_fields, unsigned long long* d_n_reached);
