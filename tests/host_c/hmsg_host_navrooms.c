/* Rooms on a free map from C through include/hmsg.h alone (N11): hmsg_nav_room_doors on a map and the rooms' seeds, then the legs of
 * a path list by room.  The first call has lists of one door and one cell: it is answered with the counts, and the call repeated.
 *   hmsg_host_navrooms <in.bin> <out.bin>
 *   in : i32 rows cols n_rooms min_clearance n_paths pad | u8 map[rows][cols] | i64 seed_off[n_rooms + 1] | i32 seed_rc[sum][2] |
 *        i64 path_off[n_paths + 1] | i32 path_rc[sum][2]
 *   out: i64 n_doors n_door_cells n_legs | i32 label[rows][cols] | u8 passable[rows][cols] | i32 other[rows][cols] |
 *        i32 door_pair[n_doors][2] | i64 door_off[n_doors + 1] | i32 door_rc[n_door_cells][2] | i32 adjacency[n_rooms][n_rooms] |
 *        i64 leg_off[n_paths + 1] | i32 leg_room[n_legs] | i64 leg_first[n_legs] */
#include <stdio.h>
#include <stdlib.h>

#include "hmsg.h"

static void* rd(FILE* f, size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (!p || (bytes && fread(p, 1, bytes, f) != bytes)) {
        fprintf(stderr, "hmsg_host_navrooms: short read (%lu bytes)\n", (unsigned long)bytes);
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
    int32_t hd[6], rows, cols, n_rooms, *seed_rc, *path_rc, *label, *leg_room;
    int64_t *seed_off, *path_off, *leg_off, *leg_first, n_paths, n_legs = 0, head[3];
    uint8_t *map, *passable;
    size_t cells;
    hmsg_route_params prm;
    hmsg_nav_door_table t;
    int rc;

    if (argc != 3) {
        fprintf(stderr, "usage: hmsg_host_navrooms <in.bin> <out.bin>   (%s)\n", hmsg_version());
        return 1;
    }
    fi = fopen(argv[1], "rb");
    if (!fi) return 1;
    if (fread(hd, 4, 6, fi) != 6) return 2;
    rows = hd[0]; cols = hd[1]; n_rooms = hd[2]; n_paths = hd[4];
    cells = (size_t)rows * (size_t)cols;
    map = (uint8_t*)rd(fi, cells);
    seed_off = (int64_t*)rd(fi, ((size_t)n_rooms + 1) * sizeof(int64_t));
    seed_rc = (int32_t*)rd(fi, (size_t)seed_off[n_rooms] * 2 * sizeof(int32_t));
    path_off = (int64_t*)rd(fi, ((size_t)n_paths + 1) * sizeof(int64_t));
    path_rc = (int32_t*)rd(fi, (size_t)path_off[n_paths] * 2 * sizeof(int32_t));
    fclose(fi);

    hmsg_route_default_params(&prm);
    prm.min_clearance = hd[3];
    label = (int32_t*)mem(cells * sizeof(int32_t));
    passable = (uint8_t*)mem(cells);
    t.other = (int32_t*)mem(cells * sizeof(int32_t));
    t.adjacency = (int32_t*)mem((size_t)n_rooms * (size_t)n_rooms * sizeof(int32_t));
    t.door_capacity = 1;                               /* too short on purpose: the first call says what is needed */
    t.cell_capacity = 1;
    t.door_pair = (int32_t*)mem(2 * sizeof(int32_t));
    t.door_off = (int64_t*)mem(2 * sizeof(int64_t));
    t.door_rc = (int32_t*)mem(2 * sizeof(int32_t));
    rc = hmsg_nav_room_doors(0, rows, cols, map, &prm, n_rooms, seed_off, seed_rc, label, passable, &t);
    if (rc != HMSG_OK && (t.n_doors > t.door_capacity || t.n_door_cells > t.cell_capacity)) {
        free(t.door_pair); free(t.door_off); free(t.door_rc);
        t.door_capacity = t.n_doors;
        t.cell_capacity = t.n_door_cells;
        t.door_pair = (int32_t*)mem((size_t)t.n_doors * 2 * sizeof(int32_t));
        t.door_off = (int64_t*)mem(((size_t)t.n_doors + 1) * sizeof(int64_t));
        t.door_rc = (int32_t*)mem((size_t)t.n_door_cells * 2 * sizeof(int32_t));
        rc = hmsg_nav_room_doors(0, rows, cols, map, &prm, n_rooms, seed_off, seed_rc, label, passable, &t);
    }
    if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_host_navrooms: hmsg_nav_room_doors -> %d\n", rc);
        return 3;
    }

    leg_off = (int64_t*)mem(((size_t)n_paths + 1) * sizeof(int64_t));
    rc = hmsg_nav_path_rooms(0, rows, cols, label, n_paths, path_off, path_rc, leg_off, NULL, NULL, 0, &n_legs);      /* the count alone */
    if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_host_navrooms: hmsg_nav_path_rooms (count) -> %d\n", rc);
        return 3;
    }
    leg_room = (int32_t*)mem((size_t)n_legs * sizeof(int32_t));
    leg_first = (int64_t*)mem((size_t)n_legs * sizeof(int64_t));
    rc = hmsg_nav_path_rooms(0, rows, cols, label, n_paths, path_off, path_rc, leg_off, leg_room, leg_first, n_legs, &n_legs);
    if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_host_navrooms: hmsg_nav_path_rooms -> %d\n", rc);
        return 3;
    }

    fo = fopen(argv[2], "wb");
    if (!fo) return 1;
    head[0] = t.n_doors; head[1] = t.n_door_cells; head[2] = n_legs;
    fwrite(head, 8, 3, fo);
    fwrite(label, 4, cells, fo);
    fwrite(passable, 1, cells, fo);
    fwrite(t.other, 4, cells, fo);
    fwrite(t.door_pair, 4, (size_t)t.n_doors * 2, fo);
    fwrite(t.door_off, 8, (size_t)t.n_doors + 1, fo);
    fwrite(t.door_rc, 4, (size_t)t.n_door_cells * 2, fo);
    fwrite(t.adjacency, 4, (size_t)n_rooms * (size_t)n_rooms, fo);
    fwrite(leg_off, 8, (size_t)n_paths + 1, fo);
    fwrite(leg_room, 4, (size_t)n_legs, fo);
    fwrite(leg_first, 8, (size_t)n_legs, fo);
    fclose(fo);
    printf("rooms %d doors %ld door cells %ld legs %ld\n", (int)n_rooms, (long)t.n_doors, (long)t.n_door_cells, (long)n_legs);
    free(map); free(seed_off); free(seed_rc); free(path_off); free(path_rc); free(label); free(passable);
    free(t.other); free(t.adjacency); free(t.door_pair); free(t.door_off); free(t.door_rc); free(leg_off); free(leg_room); free(leg_first);
    return 0;
}
