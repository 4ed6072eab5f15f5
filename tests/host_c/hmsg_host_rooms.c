/* The query applications' flow from C through include/hmsg.h alone (visualize_query_graph_icra_*.py: load_hmsg_graph,
 * generate_room_names(generate_method="obj_embedding", default_room_types=[...]), query_hierarchy_protected_icra):
 *   hmsg_load -> hmsg_graph_name_rooms -> room_name_emb from type_of_room -> label-mode hmsg_graph_query -> hmsg_graph_to_json.
 * usage: hmsg_host_rooms <graph dir> <in.bin> <out.bin> <out.json> <type name>...
 *   in.bin : int32 n_types, D, Q, C, k; f32 type_feats [n_types][D]; f32 T_obj [Q][C][D]; f32 T_room [Q][D]
 *   out.bin: int32 n_rooms, type_of_room [n_rooms]; int32 nsel [Q]; int32 sel [Q][max(n_rooms, 10)]; int32 idx [Q][k];
 *            int32 room [Q][k]; f64 score [Q][k] */
#include <stdio.h>
#include <stdlib.h>

#include "hmsg.h"

static int fail(const char* what, int rc, const hmsg_graph_t* g) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, g ? hmsg_graph_last_error(g) : "");
    return 1;
}

static int read_all(FILE* f, void* p, size_t size, size_t n) { return fread(p, size, n, f) == n; }

int main(int argc, char** argv) {
    FILE* fi;
    FILE* fo;
    int32_t hdr[5], n_types, D, Q, C, k, R, RM, q, r, d;
    float *types, *T_obj, *T_room;
    int32_t *type_of_room, *qid, *floor_id, *mode, *sel, *nsel, *idx, *room;
    double *names_emb, *score;
    hmsg_graph_t* g = NULL;
    hmsg_graph_counts cnt;
    int64_t need = 0;
    char* json;
    int rc;
    if (argc < 6) {
        fprintf(stderr, "usage: %s <graph dir> <in.bin> <out.bin> <out.json> <type name>...\n", argv[0]);
        return 2;
    }
    fi = fopen(argv[2], "rb");
    if (!fi || !read_all(fi, hdr, 4, 5)) return 2;
    n_types = hdr[0], D = hdr[1], Q = hdr[2], C = hdr[3], k = hdr[4];
    if (n_types != argc - 5) return 2;
    types = (float*)malloc((size_t)n_types * D * 4);
    T_obj = (float*)malloc((size_t)Q * C * D * 4);
    T_room = (float*)malloc((size_t)Q * D * 4);
    if (!read_all(fi, types, 4, (size_t)n_types * D) || !read_all(fi, T_obj, 4, (size_t)Q * C * D) || !read_all(fi, T_room, 4, (size_t)Q * D)) return 2;
    fclose(fi);
    /* 1. load_hmsg_graph */
    if ((rc = hmsg_load(argv[1], 0, &g)) != HMSG_OK) return fail("hmsg_load", rc, NULL);
    if ((rc = hmsg_graph_get_counts(g, &cnt)) != HMSG_OK) return fail("hmsg_graph_get_counts", rc, g);
    R = cnt.rooms;
    RM = R > 10 ? R : 10;
    /* 2. generate_room_names(generate_method="obj_embedding") */
    type_of_room = (int32_t*)malloc((size_t)(R > 0 ? R : 1) * 4);
    rc = hmsg_graph_name_rooms(g, HMSG_ROOM_NAMES_OBJ_EMBEDDING, n_types, types, (const char* const*)(argv + 5), type_of_room);
    if (rc != HMSG_OK) return fail("hmsg_graph_name_rooms", rc, g);
    /* 3. the text feature of a room's name is its type's row */
    names_emb = (double*)malloc((size_t)(R > 0 ? R : 1) * D * 8);
    for (r = 0; r < R; ++r)
        for (d = 0; d < D; ++d) names_emb[(size_t)r * D + d] = (double)types[(size_t)type_of_room[r] * D + d];
    /* 4. query_hmsg_room(..., "label") -> query_hmsg_object over its rooms */
    qid = (int32_t*)calloc((size_t)Q, 4);
    floor_id = (int32_t*)malloc((size_t)Q * 4);
    mode = (int32_t*)malloc((size_t)Q * 4);
    for (q = 0; q < Q; ++q) floor_id[q] = -1, mode[q] = 1;
    sel = (int32_t*)malloc((size_t)Q * RM * 4);
    nsel = (int32_t*)malloc((size_t)Q * 4);
    idx = (int32_t*)malloc((size_t)Q * k * 4);
    room = (int32_t*)malloc((size_t)Q * k * 4);
    score = (double*)malloc((size_t)Q * k * 8);
    rc = hmsg_graph_query(g, names_emb, Q, C, T_obj, qid, T_room, floor_id, mode, k, 1, RM, sel, nsel, idx, room, score);
    if (rc != HMSG_OK) return fail("hmsg_graph_query", rc, g);
    /* 5. the named graph */
    if ((rc = hmsg_graph_to_json(g, NULL, 0, &need)) != HMSG_OK) return fail("hmsg_graph_to_json", rc, g);
    json = (char*)malloc((size_t)need + 1);
    if ((rc = hmsg_graph_to_json(g, json, need + 1, &need)) != HMSG_OK) return fail("hmsg_graph_to_json", rc, g);
    fo = fopen(argv[4], "wb");
    if (!fo) return 2;
    fputs(json, fo);
    fclose(fo);
    fo = fopen(argv[3], "wb");
    if (!fo) return 2;
    fwrite(&R, 4, 1, fo);
    fwrite(type_of_room, 4, (size_t)R, fo);
    fwrite(nsel, 4, (size_t)Q, fo);
    fwrite(sel, 4, (size_t)Q * RM, fo);
    fwrite(idx, 4, (size_t)Q * k, fo);
    fwrite(room, 4, (size_t)Q * k, fo);
    fwrite(score, 8, (size_t)Q * k, fo);
    fclose(fo);
    hmsg_graph_destroy(g);
    free(types), free(T_obj), free(T_room), free(type_of_room), free(names_emb), free(qid), free(floor_id), free(mode);
    free(sel), free(nsel), free(idx), free(room), free(score), free(json);
    printf("hmsg_host_rooms ok: %d rooms\n", R);
    return 0;
}
