/* Routes across storeys from C through include/hmsg.h alone (N9): hmsg_nav_building_fields for one start, then
 * hmsg_nav_building_route from the same start to a list of goals.  The first route call has a path list of one cell: it is
 * answered with the count, and the call repeated.
 *   hmsg_host_building <in.bin> <out.bin>
 *   in : i32 n_storeys n_links n_goals min_clearance start[3] | i32 rows[n_storeys] | i32 cols[n_storeys] | u8 map_l[rows_l][cols_l] per
 *        storey | i32 links[n_links][7] | i32 goals[n_goals][3]
 *   out: i32 start_cell[3] | i64 start_d2 n_path_cells | i64 n_reached[n_storeys] | per storey i32 field_l (of hmsg_nav_building_fields
 *        on the maps as they are) | per storey u8 passable_l | i32 goal_cell[n][3] | i64 goal_d2[n] | i32 goal_dist[n] |
 *        i64 path_off[n + 1] | i32 path_src[n_path_cells][3] */
#include <stdio.h>
#include <stdlib.h>

#include "hmsg.h"

static void* rd(FILE* f, size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (!p || (bytes && fread(p, 1, bytes, f) != bytes)) {
        fprintf(stderr, "hmsg_host_building: short read (%lu bytes)\n", (unsigned long)bytes);
        exit(2);
    }
    return p;
}

int main(int argc, char** argv) {
    FILE *fi, *fo;
    int32_t hd[7], ns, nl, *rows, *cols, *links, *goals, **fields;
    int64_t n, tail[2], *reached;
    uint8_t **maps, **passable;
    const uint8_t** cmaps;
    hmsg_route_params prm;
    hmsg_nav_building_routes out;
    int rc, l;

    if (argc != 3) {
        fprintf(stderr, "usage: hmsg_host_building <in.bin> <out.bin>   (%s)\n", hmsg_version());
        return 1;
    }
    fi = fopen(argv[1], "rb");
    if (!fi) return 1;
    if (fread(hd, 4, 7, fi) != 7) return 2;
    ns = hd[0]; nl = hd[1]; n = hd[2];
    rows = (int32_t*)rd(fi, (size_t)ns * 4);
    cols = (int32_t*)rd(fi, (size_t)ns * 4);
    maps = (uint8_t**)malloc((size_t)ns * sizeof(uint8_t*));
    cmaps = (const uint8_t**)malloc((size_t)ns * sizeof(uint8_t*));
    passable = (uint8_t**)malloc((size_t)ns * sizeof(uint8_t*));
    fields = (int32_t**)malloc((size_t)ns * sizeof(int32_t*));
    reached = (int64_t*)malloc((size_t)ns * sizeof(int64_t));
    if (!maps || !cmaps || !passable || !fields || !reached) return 5;
    for (l = 0; l < ns; ++l) {
        size_t cells = (size_t)rows[l] * (size_t)cols[l];
        maps[l] = (uint8_t*)rd(fi, cells);
        cmaps[l] = maps[l];
        passable[l] = (uint8_t*)malloc(cells);
        fields[l] = (int32_t*)malloc(cells * sizeof(int32_t));
        if (!passable[l] || !fields[l]) return 5;
    }
    links = (int32_t*)rd(fi, (size_t)nl * 7 * sizeof(int32_t));
    goals = (int32_t*)rd(fi, (size_t)n * 3 * sizeof(int32_t));
    fclose(fi);

    hmsg_route_default_params(&prm);
    rc = hmsg_nav_building_fields(0, ns, rows, cols, cmaps, nl, links, &prm, 1, hd + 4, fields, reached);
    if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_host_building: hmsg_nav_building_fields -> %d\n", rc);
        return 3;
    }

    prm.min_clearance = hd[3];
    out.goal_cell = (int32_t*)malloc((size_t)n * 3 * sizeof(int32_t) + 1);
    out.goal_d2 = (int64_t*)malloc((size_t)n * sizeof(int64_t) + 1);
    out.goal_dist = (int32_t*)malloc((size_t)n * sizeof(int32_t) + 1);
    out.path_off = (int64_t*)malloc(((size_t)n + 1) * sizeof(int64_t));
    out.field = NULL;
    out.passable = passable;
    out.path_capacity = 1;                            /* too short on purpose: the first call says what is needed */
    out.path_src = (int32_t*)malloc(3 * sizeof(int32_t));
    if (!out.goal_cell || !out.goal_d2 || !out.goal_dist || !out.path_off || !out.path_src) return 5;
    rc = hmsg_nav_building_route(0, ns, rows, cols, cmaps, nl, links, &prm, hd + 4, n, goals, &out);
    if (rc != HMSG_OK && out.n_path_cells > out.path_capacity) {
        free(out.path_src);
        out.path_capacity = out.n_path_cells;
        out.path_src = (int32_t*)malloc((size_t)out.n_path_cells * 3 * sizeof(int32_t));
        if (!out.path_src) return 5;
        rc = hmsg_nav_building_route(0, ns, rows, cols, cmaps, nl, links, &prm, hd + 4, n, goals, &out);
    }
    if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_host_building: hmsg_nav_building_route -> %d\n", rc);
        return 3;
    }

    fo = fopen(argv[2], "wb");
    if (!fo) return 1;
    tail[0] = out.start_d2; tail[1] = out.n_path_cells;
    fwrite(out.start_cell, 4, 3, fo);
    fwrite(tail, 8, 2, fo);
    fwrite(reached, 8, (size_t)ns, fo);
    for (l = 0; l < ns; ++l) fwrite(fields[l], 4, (size_t)rows[l] * (size_t)cols[l], fo);
    for (l = 0; l < ns; ++l) fwrite(passable[l], 1, (size_t)rows[l] * (size_t)cols[l], fo);
    fwrite(out.goal_cell, 4, (size_t)n * 3, fo);
    fwrite(out.goal_d2, 8, (size_t)n, fo);
    fwrite(out.goal_dist, 4, (size_t)n, fo);
    fwrite(out.path_off, 8, (size_t)n + 1, fo);
    fwrite(out.path_src, 4, (size_t)out.n_path_cells * 3, fo);
    fclose(fo);
    printf("start (%d, %d, %d) goals %ld path cells %ld\n", (int)out.start_cell[0], (int)out.start_cell[1], (int)out.start_cell[2], (long)n,
           (long)out.n_path_cells);
    for (l = 0; l < ns; ++l) { free(maps[l]); free(passable[l]); free(fields[l]); }
    free(maps); free(cmaps); free(passable); free(fields); free(reached); free(rows); free(cols); free(links); free(goals);
    free(out.goal_cell); free(out.goal_d2); free(out.goal_dist); free(out.path_off); free(out.path_src);
    return 0;
}
