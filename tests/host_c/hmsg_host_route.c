/* Routes on a free map from C through include/hmsg.h alone (N7): the clearance of the map, then hmsg_nav_route from a start to a
 * list of goals.  The first call has a path list of one cell: it is answered with the count, and the call repeated.
 *   hmsg_host_route <in.bin> <out.bin>
 *   in : i32 rows cols n_goals min_clearance start[2] | u8 map[rows][cols] | i32 goal_rc[n_goals][2]
 *   out: i32 start_cell[2] | i64 start_d2 n_path_cells | i32 clearance[rows][cols] | u8 passable[rows][cols] | i32 goal_cell[n][2] |
 *        i64 goal_d2[n] | i32 goal_dist[n] | i64 path_off[n + 1] | i32 path_rc[n_path_cells][2] */
#include <stdio.h>
#include <stdlib.h>

#include "hmsg.h"

static void* rd(FILE* f, size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (!p || (bytes && fread(p, 1, bytes, f) != bytes)) {
        fprintf(stderr, "hmsg_host_route: short read (%lu bytes)\n", (unsigned long)bytes);
        exit(2);
    }
    return p;
}

int main(int argc, char** argv) {
    FILE *fi, *fo;
    int32_t hd[6], rows, cols, *goals, *clearance;
    int64_t n, tail[2];
    uint8_t* map;
    size_t cells;
    hmsg_route_params prm;
    hmsg_nav_routes out;
    int rc;

    if (argc != 3) {
        fprintf(stderr, "usage: hmsg_host_route <in.bin> <out.bin>   (%s)\n", hmsg_version());
        return 1;
    }
    fi = fopen(argv[1], "rb");
    if (!fi) return 1;
    if (fread(hd, 4, 6, fi) != 6) return 2;
    rows = hd[0]; cols = hd[1]; n = hd[2];
    cells = (size_t)rows * (size_t)cols;
    map = (uint8_t*)rd(fi, cells);
    goals = (int32_t*)rd(fi, (size_t)n * 2 * sizeof(int32_t));
    fclose(fi);

    hmsg_route_default_params(&prm);
    if (prm.w_straight != 5 || prm.w_diag != 7 || prm.min_clearance != 0) return 6;
    prm.min_clearance = hd[3];
    clearance = (int32_t*)malloc(cells * sizeof(int32_t));
    if (!clearance) return 5;
    rc = hmsg_nav_clearance(0, rows, cols, map, &prm, clearance);
    if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_host_route: hmsg_nav_clearance -> %d\n", rc);
        return 3;
    }

    out.goal_cell = (int32_t*)malloc((size_t)n * 2 * sizeof(int32_t) + 1);
    out.goal_d2 = (int64_t*)malloc((size_t)n * sizeof(int64_t) + 1);
    out.goal_dist = (int32_t*)malloc((size_t)n * sizeof(int32_t) + 1);
    out.path_off = (int64_t*)malloc(((size_t)n + 1) * sizeof(int64_t));
    out.field = NULL;
    out.passable = (uint8_t*)malloc(cells);
    out.path_capacity = 1;                            /* too short on purpose: the first call says what is needed */
    out.path_rc = (int32_t*)malloc(2 * sizeof(int32_t));
    if (!out.goal_cell || !out.goal_d2 || !out.goal_dist || !out.path_off || !out.passable || !out.path_rc) return 5;
    rc = hmsg_nav_route(0, rows, cols, map, &prm, hd + 4, n, goals, &out);
    if (rc != HMSG_OK && out.n_path_cells > out.path_capacity) {
        free(out.path_rc);
        out.path_capacity = out.n_path_cells;
        out.path_rc = (int32_t*)malloc((size_t)out.n_path_cells * 2 * sizeof(int32_t));
        if (!out.path_rc) return 5;
        rc = hmsg_nav_route(0, rows, cols, map, &prm, hd + 4, n, goals, &out);
    }
    if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_host_route: hmsg_nav_route -> %d\n", rc);
        return 3;
    }

    fo = fopen(argv[2], "wb");
    if (!fo) return 1;
    tail[0] = out.start_d2; tail[1] = out.n_path_cells;
    fwrite(out.start_cell, 4, 2, fo);
    fwrite(tail, 8, 2, fo);
    fwrite(clearance, 4, cells, fo);
    fwrite(out.passable, 1, cells, fo);
    fwrite(out.goal_cell, 4, (size_t)n * 2, fo);
    fwrite(out.goal_d2, 8, (size_t)n, fo);
    fwrite(out.goal_dist, 4, (size_t)n, fo);
    fwrite(out.path_off, 8, (size_t)n + 1, fo);
    fwrite(out.path_rc, 4, (size_t)out.n_path_cells * 2, fo);
    fclose(fo);
    printf("start (%d, %d) goals %ld path cells %ld\n", (int)out.start_cell[0], (int)out.start_cell[1], (long)n, (long)out.n_path_cells);
    free(map); free(goals); free(clearance);
    free(out.goal_cell); free(out.goal_d2); free(out.goal_dist); free(out.path_off); free(out.passable); free(out.path_rc);
    return 0;
}
