/* Sight over furniture from C through include/hmsg.h alone (N10): hmsg_nav_grid says the size, hmsg_nav_height_map makes the
 * storey's height map, the host takes the cells that are known and no higher than max_step as the map to walk on, then
 * hmsg_nav_view_route_h from a start to a list of goals and hmsg_nav_viewpoints_h on the passable map and the field that call
 * returned, with the masks.  The first route call has a path list of one cell: it is answered with the count, and the call
 * repeated when that is larger.
 *   hmsg_host_sight <in.bin> <out.bin>
 *   in : i64 n_points n_goals | f64 zero_level cell_size height_unit top_max | i32 dilation max_step eye min_clearance start[2] |
 *        i64 r_min2 r_max2 | f64 xyz[n_points][3] | i32 goal_rc[n_goals][2] | i32 goal_h[n_goals] | i64 goal_r2[n_goals]
 *   out: i32 grid[2] start_cell[2] | i64 start_d2 n_path_cells | u16 top[rows][cols] | u8 known[rows][cols] |
 *        u8 passable[rows][cols] | i32 goal_cell[n][2] | i64 goal_d2[n] | i32 goal_dist[n] | i32 n_visible[n] | i64 path_off[n + 1] |
 *        i32 path_rc[n_path_cells][2] | i32 view_rc[n][2] | i64 view_d2[n] | i32 view_dist[n] | i32 view_n_visible[n] |
 *        u8 visible[n][rows][cols] */
#include <stdio.h>
#include <stdlib.h>

#include "hmsg.h"

static void* rd(FILE* f, size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (!p || (bytes && fread(p, 1, bytes, f) != bytes)) {
        fprintf(stderr, "hmsg_host_sight: short read (%lu bytes)\n", (unsigned long)bytes);
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
    int64_t cnt[2], n, band[2], tail[2], *goal_r2, *view_d2;
    double f4[4], *xyz, pcd_min[3], pcd_max[3];
    int32_t i6[6], grid[2], again[2], rows, cols, *goals, *goal_h, *n_visible, *view_rc, *view_dist, *view_n;
    uint16_t* top;
    uint8_t *known, *map, *visible;
    size_t cells, i;
    hmsg_height_params hp;
    hmsg_route_params prm;
    hmsg_view_params vp;
    hmsg_nav_routes out;
    int rc;

    if (argc != 3) {
        fprintf(stderr, "usage: hmsg_host_sight <in.bin> <out.bin>   (%s)\n", hmsg_version());
        return 1;
    }
    fi = fopen(argv[1], "rb");
    if (!fi) return 1;
    if (fread(cnt, 8, 2, fi) != 2 || fread(f4, 8, 4, fi) != 4 || fread(i6, 4, 6, fi) != 6 || fread(band, 8, 2, fi) != 2) return 2;
    n = cnt[1];
    xyz = (double*)rd(fi, (size_t)cnt[0] * 3 * sizeof(double));
    goals = (int32_t*)rd(fi, (size_t)n * 2 * sizeof(int32_t));
    goal_h = (int32_t*)rd(fi, (size_t)n * sizeof(int32_t));
    goal_r2 = (int64_t*)rd(fi, (size_t)n * sizeof(int64_t));
    fclose(fi);

    hmsg_height_default_params(&hp);
    if (hp.cell_size != 0.03 || hp.height_unit != 0.01 || hp.top_max != 2.5 || hp.dilation != 5) return 6;
    hp.cell_size = f4[1]; hp.height_unit = f4[2]; hp.top_max = f4[3]; hp.dilation = i6[0];
    rc = hmsg_nav_grid(0, hp.cell_size, cnt[0], xyz, NULL, NULL, grid);
    if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_host_sight: hmsg_nav_grid -> %d\n", rc);
        return 3;
    }
    cols = grid[0]; rows = grid[1];
    cells = (size_t)rows * (size_t)cols;
    top = (uint16_t*)mem(cells * sizeof(uint16_t));
    known = (uint8_t*)mem(cells);
    rc = hmsg_nav_height_map(0, &hp, cnt[0], xyz, f4[0], top, known, pcd_min, pcd_max, again);
    if (rc != HMSG_OK || again[0] != grid[0] || again[1] != grid[1] || pcd_min[0] > pcd_max[0]) {
        fprintf(stderr, "hmsg_host_sight: hmsg_nav_height_map -> %d\n", rc);
        return 3;
    }
    map = (uint8_t*)mem(cells);
    for (i = 0; i < cells; ++i) map[i] = (uint8_t)(known[i] && (int32_t)top[i] <= i6[1]);

    hmsg_route_default_params(&prm);
    prm.min_clearance = i6[3];
    hmsg_view_default_params(&vp);
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
    rc = hmsg_nav_view_route_h(0, rows, cols, map, top, &prm, &vp, i6[2], i6 + 4, n, goals, goal_h, goal_r2, &out, n_visible);
    if (rc != HMSG_OK && out.n_path_cells > out.path_capacity) {
        free(out.path_rc);
        out.path_capacity = out.n_path_cells;
        out.path_rc = (int32_t*)mem((size_t)out.n_path_cells * 2 * sizeof(int32_t));
        rc = hmsg_nav_view_route_h(0, rows, cols, map, top, &prm, &vp, i6[2], i6 + 4, n, goals, goal_h, goal_r2, &out, n_visible);
    }
    if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_host_sight: hmsg_nav_view_route_h -> %d\n", rc);
        return 3;
    }

    view_rc = (int32_t*)mem((size_t)n * 2 * sizeof(int32_t));
    view_d2 = (int64_t*)mem((size_t)n * sizeof(int64_t));
    view_dist = (int32_t*)mem((size_t)n * sizeof(int32_t));
    view_n = (int32_t*)mem((size_t)n * sizeof(int32_t));
    visible = (uint8_t*)mem((size_t)n * cells);
    rc = hmsg_nav_viewpoints_h(0, rows, cols, top, out.passable, out.field, &vp, i6[2], n, goals, goal_h, goal_r2, view_rc, view_d2, view_dist,
                               view_n, visible);
    if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_host_sight: hmsg_nav_viewpoints_h -> %d\n", rc);
        return 3;
    }

    fo = fopen(argv[2], "wb");
    if (!fo) return 1;
    tail[0] = out.start_d2; tail[1] = out.n_path_cells;
    fwrite(grid, 4, 2, fo);
    fwrite(out.start_cell, 4, 2, fo);
    fwrite(tail, 8, 2, fo);
    fwrite(top, 2, cells, fo);
    fwrite(known, 1, cells, fo);
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
    printf("grid %d x %d start (%d, %d) goals %ld path cells %ld\n", (int)rows, (int)cols, (int)out.start_cell[0], (int)out.start_cell[1], (long)n,
           (long)out.n_path_cells);
    free(xyz); free(goals); free(goal_h); free(goal_r2); free(top); free(known); free(map); free(n_visible);
    free(out.goal_cell); free(out.goal_d2); free(out.goal_dist); free(out.path_off); free(out.field); free(out.passable); free(out.path_rc);
    free(view_rc); free(view_d2); free(view_dist); free(view_n); free(visible);
    return 0;
}
