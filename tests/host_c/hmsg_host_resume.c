/* The resume order of the reference's build applications from C through include/hmsg.h alone (semantic_scene_reconstruction.py:114-127:
 * load_full_pcd, load_full_pcd_feats, load_masked_pcds_new, build_hier_multimodal_scene_graph):
 *   hmsg_read_ply of full_pcd.ply and objects/pcd_<i>.ply -> hmsg_restore_stage -> hmsg_build_graph -> hmsg_save.
 * No frame is replayed.  A C host cannot read the .pt files of save_full_pcd_feats, so features, poses and the frames' global features
 * come as raw little-endian files.
 * usage: hmsg_host_resume <artefact dir> <in.bin> <out graph dir>
 *   <artefact dir>/full_pcd.ply, <artefact dir>/objects/pcd_<i>.ply for i = 0 .. N-1
 *   in.bin: int32 D, N, F, W, H, num_views; f64 voxel_size; f64 K [9]; f32 inst_feats [N][D]; f64 poses [F][16];
 *           f64 poses_inv [F][16]; f32 view_feats [F][D]; then F image paths, each int32 length + bytes */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hmsg.h"

static int read_all(FILE* f, void* p, size_t size, size_t n) { return n == 0 || fread(p, size, n, f) == n; }

int main(int argc, char** argv) {
    FILE* fi;
    int32_t hdr[6], D, N, F, W, H, i;
    double vs, K[9], *map_xyz, *inst_xyz, *poses, *poses_inv;
    float *inst_feats, *view_feats;
    int64_t V = 0, total = 0, n = 0, *off;
    char** paths;
    char name[4096];
    hmsg_config cfg;
    hmsg_graph_params prm;
    hmsg_graph_counts cnt;
    hmsg_t* h = NULL;
    hmsg_graph_t* g = NULL;
    int rc;
    if (argc != 4) {
        fprintf(stderr, "usage: %s <artefact dir> <in.bin> <out graph dir>\n", argv[0]);
        return 2;
    }
    fi = fopen(argv[2], "rb");
    if (!fi || !read_all(fi, hdr, 4, 6) || !read_all(fi, &vs, 8, 1) || !read_all(fi, K, 8, 9)) return 2;
    D = hdr[0], N = hdr[1], F = hdr[2], W = hdr[3], H = hdr[4];
    if (D <= 0 || N < 0 || F <= 0 || W <= 0 || H <= 0 || strlen(argv[1]) > 3900) return 2;
    inst_feats = (float*)malloc((size_t)(N > 0 ? N : 1) * D * 4);
    poses = (double*)malloc((size_t)F * 16 * 8);
    poses_inv = (double*)malloc((size_t)F * 16 * 8);
    view_feats = (float*)malloc((size_t)F * D * 4);
    paths = (char**)calloc((size_t)F, sizeof(char*));
    if (!inst_feats || !poses || !poses_inv || !view_feats || !paths) return 2;
    if (!read_all(fi, inst_feats, 4, (size_t)N * D) || !read_all(fi, poses, 8, (size_t)F * 16) || !read_all(fi, poses_inv, 8, (size_t)F * 16) ||
        !read_all(fi, view_feats, 4, (size_t)F * D))
        return 2;
    for (i = 0; i < F; ++i) {
        int32_t len;
        if (!read_all(fi, &len, 4, 1) || len < 0 || len > 4096) return 2;
        paths[i] = (char*)calloc((size_t)len + 1, 1);
        if (!paths[i] || !read_all(fi, paths[i], 1, (size_t)len)) return 2;
    }
    fclose(fi);
    /* 1. load_full_pcd */
    sprintf(name, "%s/full_pcd.ply", argv[1]);
    if ((rc = hmsg_read_ply(name, NULL, 0, &V)) != HMSG_OK) {
        fprintf(stderr, "hmsg_read_ply(%s) failed (%d)\n", name, rc);
        return 1;
    }
    map_xyz = (double*)malloc((size_t)(V > 0 ? V : 1) * 24);
    if (!map_xyz || (rc = hmsg_read_ply(name, map_xyz, V, &V)) != HMSG_OK) return 1;
    /* 2. load_masked_pcds_new: sizes first, then the points into one block */
    off = (int64_t*)calloc((size_t)N + 1, 8);
    if (!off) return 2;
    for (i = 0; i < N; ++i) {
        sprintf(name, "%s/objects/pcd_%d.ply", argv[1], (int)i);
        if ((rc = hmsg_read_ply(name, NULL, 0, &n)) != HMSG_OK) {
            fprintf(stderr, "hmsg_read_ply(%s) failed (%d)\n", name, rc);
            return 1;
        }
        off[i + 1] = off[i] + n;
    }
    total = off[N];
    inst_xyz = (double*)malloc((size_t)(total > 0 ? total : 1) * 24);
    if (!inst_xyz) return 2;
    for (i = 0; i < N; ++i) {
        sprintf(name, "%s/objects/pcd_%d.ply", argv[1], (int)i);
        if ((rc = hmsg_read_ply(name, inst_xyz + (size_t)off[i] * 3, off[i + 1] - off[i], &n)) != HMSG_OK || n != off[i + 1] - off[i]) return 1;
    }
    /* 3. the scene back in HBM */
    hmsg_default_config(&cfg);
    cfg.feat_dim = D;
    cfg.width = W;
    cfg.height = H;
    cfg.max_frames = 1;
    cfg.voxel_size = vs;
    if ((rc = hmsg_create(&cfg, &h)) != HMSG_OK) {
        fprintf(stderr, "hmsg_create failed (%d)\n", rc);
        return 1;
    }
    if ((rc = hmsg_restore_stage(h, V, map_xyz, NULL, NULL, N, off, inst_xyz, inst_feats, K)) != HMSG_OK) {
        fprintf(stderr, "hmsg_restore_stage failed (%d): %s\n", rc, hmsg_last_error(h));
        return 1;
    }
    /* 4. build_hier_multimodal_scene_graph + save_hmsg_graph */
    hmsg_graph_default_params(&prm);
    prm.num_views = hdr[5];
    prm.host_threads = 2;
    rc = hmsg_build_graph(h, &prm, F, poses, poses_inv, view_feats, (const char* const*)paths, 0, NULL, NULL, &g);
    if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_build_graph failed (%d): %s\n", rc, hmsg_last_error(h));
        return 1;
    }
    if ((rc = hmsg_save(g, argv[3])) != HMSG_OK || (rc = hmsg_graph_get_counts(g, &cnt)) != HMSG_OK) {
        fprintf(stderr, "hmsg_save failed (%d): %s\n", rc, hmsg_graph_last_error(g));
        return 1;
    }
    printf("map %lld points, %d instances with %lld points\n", (long long)V, (int)N, (long long)total);
    printf("hmsg_host_resume ok: %d floors, %d rooms, %d views, %d objects, %lld edges, %lld view-object links\n", (int)cnt.floors, (int)cnt.rooms,
           (int)cnt.views, (int)cnt.objects, (long long)cnt.edges, (long long)cnt.view_object_links);
    hmsg_graph_destroy(g);
    hmsg_destroy(h);
    for (i = 0; i < F; ++i) free(paths[i]);
    free(paths), free(inst_feats), free(poses), free(poses_inv), free(view_feats), free(map_xyz), free(inst_xyz), free(off);
    return 0;
}
