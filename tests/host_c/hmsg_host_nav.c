/* The navigation maps of a storey from C through include/hmsg.h alone (the image half of the reference's NavigationGraph): a small
 * scene is built as the other C hosts build one -- frames, map, encoder outputs, fusion, merge, pooling --, then the graph
 * (hmsg_build_graph), then the free map and the boundary cells of floor 0: hmsg_graph_nav_grid sizes the arrays,
 * hmsg_graph_nav_floor_maps fills them; a boundary list that is too short is answered with the count, and the call repeated.
 *   hmsg_host_nav <in.bin> <out.bin>
 *   in : i32 F H W M D P outlier_nb feat_dbscan_min outlier_radius_mm cell_mm | f64 K[9] | u8 rgb[F][H][W][3] | u16 depth[F][H][W] |
 *        f64 pose[F][16] | u8 masks[F][M][H][W] | i32 n_masks[F] | f32 f_g[F][D] | f32 f_masked[F][M][D] | f32 f_crop[F][M][D] |
 *        f64 nav_pose[P][16]
 *   out: i32 grid[2] n_regions main_label | i64 main_area n_boundary | f64 pcd_min[3] pcd_max[3] | f32 obstacle_map[H'][W'] |
 *        u8 free_map[H'][W'] | u8 main_free_map[H'][W'] | u8 top_down_bgr[H'][W'][3] | i32 boundary_rc[n_boundary][2] */
#include <stdio.h>
#include <stdlib.h>

#include "hmsg.h"

static void* rd(FILE* f, size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (!p || (bytes && fread(p, 1, bytes, f) != bytes)) {
        fprintf(stderr, "hmsg_host_nav: short read (%lu bytes)\n", (unsigned long)bytes);
        exit(2);
    }
    return p;
}

#define CK(call)                                                                              \
    do {                                                                                      \
        int rc_ = (call);                                                                     \
        if (rc_ != HMSG_OK) {                                                                 \
            fprintf(stderr, "hmsg_host_nav: %s -> %d: %s\n", #call, rc_, hmsg_last_error(h)); \
            return 3;                                                                         \
        }                                                                                     \
    } while (0)
#define CKG(call)                                                                                   \
    do {                                                                                            \
        int rc_ = (call);                                                                           \
        if (rc_ != HMSG_OK) {                                                                       \
            fprintf(stderr, "hmsg_host_nav: %s -> %d: %s\n", #call, rc_, hmsg_graph_last_error(g)); \
            return 3;                                                                               \
        }                                                                                           \
    } while (0)

int main(int argc, char** argv) {
    FILE *fi, *fo;
    int32_t hd[10], F, H, W, M, D, P, grid[2], head[4];
    int64_t tail[2];
    double *K, *pose, *nav_pose, mn[3], mx[3];
    uint8_t *rgb, *masks;
    uint16_t* depth;
    int32_t* n_masks;
    float *f_g, *f_masked, *f_crop;
    hmsg_config cfg;
    hmsg_t* h = NULL;
    hmsg_graph_t* g = NULL;
    hmsg_graph_params gp;
    hmsg_nav_params np;
    hmsg_nav_maps maps;
    size_t HW, cells;
    int rc;

    if (argc != 3) {
        fprintf(stderr, "usage: hmsg_host_nav <in.bin> <out.bin>   (%s)\n", hmsg_version());
        return 1;
    }
    fi = fopen(argv[1], "rb");
    if (!fi) return 1;
    if (fread(hd, 4, 10, fi) != 10) return 2;
    F = hd[0]; H = hd[1]; W = hd[2]; M = hd[3]; D = hd[4]; P = hd[5];
    HW = (size_t)H * (size_t)W;
    K = (double*)rd(fi, 9 * sizeof(double));
    rgb = (uint8_t*)rd(fi, (size_t)F * HW * 3);
    depth = (uint16_t*)rd(fi, (size_t)F * HW * 2);
    pose = (double*)rd(fi, (size_t)F * 16 * sizeof(double));
    masks = (uint8_t*)rd(fi, (size_t)F * (size_t)M * HW);
    n_masks = (int32_t*)rd(fi, (size_t)F * 4);
    f_g = (float*)rd(fi, (size_t)F * (size_t)D * 4);
    f_masked = (float*)rd(fi, (size_t)F * (size_t)M * (size_t)D * 4);
    f_crop = (float*)rd(fi, (size_t)F * (size_t)M * (size_t)D * 4);
    nav_pose = (double*)rd(fi, (size_t)P * 16 * sizeof(double));
    fclose(fi);

    hmsg_default_config(&cfg);
    cfg.device_id = 0;
    cfg.feat_dim = D;
    cfg.height = H;
    cfg.width = W;
    cfg.max_frames = F;
    cfg.max_masks = M;
    cfg.outlier_nb_points = hd[6];
    cfg.feat_dbscan_min = hd[7];
    cfg.outlier_radius = (double)hd[8] / 1000.0;
    if (hmsg_create(&cfg, &h) != HMSG_OK || !h) {
        fprintf(stderr, "hmsg_host_nav: hmsg_create failed: %s\n", hmsg_last_error(NULL));
        return 4;
    }
    CK(hmsg_add_frames(h, F, rgb, depth, pose, K));
    CK(hmsg_finalize_map(h));
    CK(hmsg_add_frame_features(h, 0, F, M, masks, f_g, f_masked, f_crop, n_masks));
    CK(hmsg_fuse_frames(h));
    CK(hmsg_merge_instances(h));
    CK(hmsg_pool_instances(h));
    hmsg_graph_default_params(&gp);
    gp.num_views = 3;
    gp.host_threads = 1;
    CK(hmsg_build_graph(h, &gp, F, pose, NULL, f_g, NULL, 0, NULL, NULL, &g));

    hmsg_nav_default_params(&np);
    np.cell_size = (double)hd[9] / 1000.0;
    CKG(hmsg_graph_nav_grid(g, 0, np.cell_size, mn, mx, grid));
    cells = (size_t)grid[0] * (size_t)grid[1];
    maps.obstacle_map = (float*)malloc(cells * sizeof(float));
    maps.region_map = NULL;
    maps.poses_map = NULL;
    maps.free_map = (uint8_t*)malloc(cells);
    maps.main_free_map = (uint8_t*)malloc(cells);
    maps.top_down_bgr = (uint8_t*)malloc(cells * 3);
    maps.boundary_capacity = 1;                       /* too short on purpose: the first call says what is needed */
    maps.boundary_rc = (int32_t*)malloc(2 * sizeof(int32_t));
    if (!maps.obstacle_map || !maps.free_map || !maps.main_free_map || !maps.top_down_bgr || !maps.boundary_rc) return 5;
    rc = hmsg_graph_nav_floor_maps(g, 0, &np, P, nav_pose, &maps);
    if (rc != HMSG_OK && maps.n_boundary > maps.boundary_capacity) {
        free(maps.boundary_rc);
        maps.boundary_capacity = maps.n_boundary;
        maps.boundary_rc = (int32_t*)malloc((size_t)maps.n_boundary * 2 * sizeof(int32_t));
        if (!maps.boundary_rc) return 5;
        CKG(hmsg_graph_nav_floor_maps(g, 0, &np, P, nav_pose, &maps));
    } else if (rc != HMSG_OK) {
        fprintf(stderr, "hmsg_host_nav: hmsg_graph_nav_floor_maps -> %d: %s\n", rc, hmsg_graph_last_error(g));
        return 3;
    }
    if (maps.grid[0] != grid[0] || maps.grid[1] != grid[1]) return 6;

    fo = fopen(argv[2], "wb");
    if (!fo) return 1;
    head[0] = grid[0]; head[1] = grid[1]; head[2] = maps.n_regions; head[3] = maps.main_label;
    tail[0] = maps.main_area; tail[1] = maps.n_boundary;
    fwrite(head, 4, 4, fo);
    fwrite(tail, 8, 2, fo);
    fwrite(maps.pcd_min, sizeof(double), 3, fo);
    fwrite(maps.pcd_max, sizeof(double), 3, fo);
    fwrite(maps.obstacle_map, sizeof(float), cells, fo);
    fwrite(maps.free_map, 1, cells, fo);
    fwrite(maps.main_free_map, 1, cells, fo);
    fwrite(maps.top_down_bgr, 1, cells * 3, fo);
    fwrite(maps.boundary_rc, 4, (size_t)maps.n_boundary * 2, fo);
    fclose(fo);
    printf("grid %d x %d regions %d main_label %d main_area %ld boundary %ld\n", (int)grid[0], (int)grid[1], (int)maps.n_regions,
           (int)maps.main_label, (long)maps.main_area, (long)maps.n_boundary);
    hmsg_graph_destroy(g);
    hmsg_destroy(h);
    free(K); free(rgb); free(depth); free(pose); free(masks); free(n_masks); free(f_g); free(f_masked); free(f_crop); free(nav_pose);
    free(maps.obstacle_map); free(maps.free_map); free(maps.main_free_map); free(maps.top_down_bgr); free(maps.boundary_rc);
    return 0;
}
