/* Viewpoints from C through include/hmsg.h alone (N8): hmsg_nav_view_route from a start to a list of goals, then
 * hmsg_nav_viewpoints on the passable map and the field that call returned, with the masks.  The first route call has a path list of
 * one cell: it is answered with the count, and the call repeated when that is larger.
 *   hmsg_host_view <in.bin> <out.bin>
 *   in : i32 rows cols n_goals min_clearance start[2] | i64 r_min2 r_max2 | u8 map[rows][cols] | u8 blocking[rows][cols] |
 *        i32 goal_rc[n_goals][2]
 *   out: i32 start_cell[2] | i64 start_d2 n_path_cells | u8 passable[rows][cols] | i32 goal_cell[n][2] | i64 goal_d2[n] |
 *        i32 goal_dist[n] | i32 n_visible[n] | i64 path_off[n + 1] | i32 path_rc[n_path_cells][2] |
 *        i32 view_rc[n][2] | i64 view_d2[n] | i32 view_dist[n] | i32 view_n_visible[n] | u8 visible[n][rows][cols] */
#include <stdio.h>
#include <stdlib.h>

#include "hmsg.h"

static void* rd(FILE* f, size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (!p || (bytes && fread(p, 1, bytes, f) != bytes)) {
        fprintf(stderr, "hmsg_host_view: short read (%lu bytes)\n", (unsigned long)bytes);
        exit(2);
    }
    return p;
}

static void* mem(size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (!p) exit(5);
    return p;
}

int main(int argc, char** argv) {
    FILE *fi, *fo;
    int32_t hd[6], rows, cols, *goals, *n_visible, *view_rc, *view_dist, *view_n;
    int64_t n, band[2], tail[2], *view_d2;
    uint8_t *map, *blocking, *visible;
    size_t cells;
    hmsg_route_params prm;
    hmsg_view_params vp;
    hmsg_nav_routes out;
    int rc;

    if (argc != 3) {
        fprintf(stderr, "usage: hmsg_host_view <in.bin> <out.bin>   (%s)\n", hmsg_version());
        return 1;
    }
    fi = fopen(argv[1], "rb");
    if (!fi) return 1;
    if (fread(hd, 4, 6, fi) != 6 || fread(band, 8, 2, fi) != 2) return 2;
    rows = hd[0]; cols = hd[1]; n = hd[2];
    cells = (size_t)rows * (size_t)cols;
    map = (uint8_t*)rd(fi, cells);
    blocking = (uint8_t*)rd(fi, cells);
    goals = (int32_t*)rd(fi, (size_t)n * 2 * sizeof(int32_t));
    fclose(fi);

    hmsg_route_default_params(&prm);
    prm.min_clearance = hd[3];
    hmsg_view_default_params(&vp);
    if (vp.r_min2 != 0 || vp.r_max2 != 100 * 100 || vp.prefer != 0) return 6;
    vp.r_min2 = band[0]; vp.r_max2 = band[1];

    out.goal_cell = (int32_t*)mem((size_t)n * 2 * sizeof(int32_t));
    out.goal_d2 = (int64_t*)mem((size_t)n * sizeof(int64_t));
    out.goal_dist = (int32_t*)mem((size_t)n * sizeof(int32_t));
    out.path_off = (int64_t*)mem(((size_t)n + 1) * sizeof(int64_t));
    out.field = (int32_t*)mem(cells * sizeof(int32_t));
    out.passable = (uint8_t*)mem(cells);
    out.path_capacity = 1;                            /* too short unless every path is empty: the first call says what is needed */
    out.path_rc = (int32_t*)mem(2 * sizeof(int32_t));
    n_visible = (int32_t*)mem((size_t)n * sizeof(int32_t));
    rc = hmsg_nav_view_route(0, rows, cols, map, blocking, &prm, &vp, hd + 4, n, goals, &out, n_visible);
    if (rc != HMSG_OK && out.n_path_cells > out.path_capacity) {
        free(out.path_rc);
        out.path_capacity = out.n_path_cells;
        out.path_rc = (int32_t*)mem((size_t)out.n_path_cells * 2 * sizeof(int32_t));
        rc = hmsg_nav_view_route(0, rows, cols, map, blocking, &prm, &vp, hd + 4, n, goals, &out, n_visible);
    }
    if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_host_view: hmsg_nav_view_route -> %d\n", rc);
        return 3;
    }

    view_rc = (int32_t*)mem((size_t)n * 2 * sizeof(int32_t));
    view_d2 = (int64_t*)mem((size_t)n * sizeof(int64_t));
    view_dist = (int32_t*)mem((size_t)n * sizeof(int32_t));
    view_n = (int32_t*)mem((size_t)n * sizeof(int32_t));
    visible = (uint8_t*)mem((size_t)n * cells);
    rc = hmsg_nav_viewpoints(0, rows, cols, blocking, out.passable, out.field, &vp, n, goals, view_rc, view_d2, view_dist, view_n, visible);
    if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_host_view: hmsg_nav_viewpoints -> %d\n", rc);
        return 3;
    }

    fo = fopen(argv[2], "wb");
    if (!fo) return 1;
    tail[0] = out.start_d2; tail[1] = out.n_path_cells;
    fwrite(out.start_cell, 4, 2, fo);
    fwrite(tail, 8, 2, fo);
    fwrite(out.passable, 1, cells, fo);
    fwrite(out.goal_cell, 4, (size_t)n * 2, fo);
    fwrite(out.goal_d2, 8, (size_t)n, fo);
    fwrite(out.goal_dist, 4, (size_t)n, fo);
    fwrite(n_visible, 4, (size_t)n, fo);
    fwrite(out.path_off, 8, (size_t)n + 1, fo);
    fwrite(out.path_rc, 4, (size_t)out.n_path_cells * 2, fo);
    fwrite(view_rc, 4, (size_t)n * 2, fo);
    fwrite(view_d2, 8, (size_t)n, fo);
    fwrite(view_dist, 4, (size_t)n, fo);
    fwrite(view_n, 4, (size_t)n, fo);
    fwrite(visible, 1, (size_t)n * cells, fo);
    fclose(fo);
    printf("start (%d, %d) goals %ld path cells %ld\n", (int)out.start_cell[0], (int)out.start_cell[1], (long)n, (long)out.n_path_cells);
    free(map); free(blocking); free(goals); free(n_visible);
    free(out.goal_cell); free(out.goal_d2); free(out.goal_dist); free(out.path_off); free(out.field); free(out.passable); free(out.path_rc);
    free(view_rc); free(view_d2); free(view_dist); free(view_n); free(visible);
    return 0;
}
