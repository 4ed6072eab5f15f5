/* A plain C99 host that hands a frame's masks over as SAM's uncompressed run-length records: compiled with
 * `gcc -std=c99 -pedantic -Wall -Wextra -Werror` against include/hmsg.h ALONE and linked with the library
 * (tests/test_rle_masks.py, tests/test_rle_masks_gpu.py).  hmsg_add_frames, hmsg_add_frame_features_rle in two hand-overs, fusion,
 * merge and pooling; it prints the instance count and the instances' sizes, and the test compares them with a dense build of the
 * same scene through the Python binding.
 *
 *   hmsg_host_rle <in.bin>
 *   in : i32 F H W M D outlier_nb feat_dbscan_min outlier_radius_mm voxel_size_mm 0 | i64 T | i64 n_counts | f64 K[9] | u8 rgb[F][H][W][3] |
 *        u16 depth[F][H][W] | f64 pose[F][16] | i32 n_masks[F] | i64 run_off[T + 1] | u32 counts[n_counts] | f32 f_g[F][D] |
 *        f32 f_masked[F][M][D] | f32 f_crop[F][M][D]
 *   out: "instances <N>" and one line "size <n>" per instance on stdout */
#include <stdio.h>
#include <stdlib.h>

#include "hmsg.h"

static void* rd(FILE* f, size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (!p || (bytes && fread(p, 1, bytes, f) != bytes)) {
        fprintf(stderr, "hmsg_host_rle: short read (%lu bytes)\n", (unsigned long)bytes);
        exit(2);
    }
    return p;
}

#define CK(call)                                                                              \
    do {                                                                                      \
        int rc_ = (call);                                                                     \
        if (rc_ != HMSG_OK) {                                                                 \
            fprintf(stderr, "hmsg_host_rle: %s -> %d: %s\n", #call, rc_, hmsg_last_error(h)); \
            return 3;                                                                         \
        }                                                                                     \
    } while (0)

int main(int argc, char** argv) {
    FILE* fi;
    int32_t hd[10], F, H, W, M, D, f, half, t_half = 0;
    int64_t hd2[2], T, n_counts, N, i, *run_off, *run_off2, *sizes;
    double *K, *pose;
    uint8_t* rgb;
    uint16_t* depth;
    int32_t* n_masks;
    uint32_t* counts;
    float *f_g, *f_masked, *f_crop;
    hmsg_config cfg;
    hmsg_t* h = NULL;
    size_t HW;

    if (argc != 2) {
        fprintf(stderr, "usage: hmsg_host_rle <in.bin>   (%s)\n", hmsg_version());
        return 1;
    }
    fi = fopen(argv[1], "rb");
    if (!fi) return 1;
    if (fread(hd, 4, 10, fi) != 10 || fread(hd2, 8, 2, fi) != 2) return 2;
    F = hd[0]; H = hd[1]; W = hd[2]; M = hd[3]; D = hd[4];
    T = hd2[0]; n_counts = hd2[1];
    HW = (size_t)H * (size_t)W;
    K = (double*)rd(fi, 9 * sizeof(double));
    rgb = (uint8_t*)rd(fi, (size_t)F * HW * 3);
    depth = (uint16_t*)rd(fi, (size_t)F * HW * 2);
    pose = (double*)rd(fi, (size_t)F * 16 * sizeof(double));
    n_masks = (int32_t*)rd(fi, (size_t)F * 4);
    run_off = (int64_t*)rd(fi, (size_t)(T + 1) * 8);
    counts = (uint32_t*)rd(fi, (size_t)n_counts * 4);
    f_g = (float*)rd(fi, (size_t)F * (size_t)D * 4);
    f_masked = (float*)rd(fi, (size_t)F * (size_t)M * (size_t)D * 4);
    f_crop = (float*)rd(fi, (size_t)F * (size_t)M * (size_t)D * 4);
    fclose(fi);

    hmsg_default_config(&cfg);
    cfg.device_id = 0;
    cfg.feat_dim = D;
    cfg.height = H;
    cfg.width = W;
    cfg.max_frames = F;
    cfg.max_masks = M;
    cfg.outlier_radius = (double)hd[7] / 1000.0;
    cfg.voxel_size = (double)hd[8] / 1000.0;
    cfg.outlier_nb_points = hd[5];
    cfg.feat_dbscan_min = hd[6];
    if (hmsg_create(&cfg, &h) != HMSG_OK || !h) {
        fprintf(stderr, "hmsg_host_rle: hmsg_create failed: %s\n", hmsg_last_error(NULL));
        return 4;
    }
    CK(hmsg_add_frames(h, F, rgb, depth, pose, K));
    CK(hmsg_finalize_map(h));
    /* two hand-overs (a service streams them): the second one's offsets start again at 0 */
    half = F / 2;
    for (f = 0; f < half; ++f) t_half += n_masks[f];
    run_off2 = (int64_t*)malloc((size_t)(T - t_half + 1) * 8);
    if (!run_off2) return 2;
    for (i = 0; i <= T - t_half; ++i) run_off2[i] = run_off[t_half + i] - run_off[t_half];
    CK(hmsg_add_frame_features_rle(h, 0, half, M, counts, run_off, n_masks, f_g, f_masked, f_crop));
    CK(hmsg_add_frame_features_rle(h, half, F - half, M, counts + run_off[t_half], run_off2, n_masks + half, f_g + (size_t)half * (size_t)D,
                                   f_masked + (size_t)half * (size_t)M * (size_t)D, f_crop + (size_t)half * (size_t)M * (size_t)D));
    CK(hmsg_fuse_frames(h));
    CK(hmsg_merge_instances(h));
    CK(hmsg_pool_instances(h));
    N = hmsg_num_instances(h);
    sizes = (int64_t*)malloc((size_t)(N ? N : 1) * sizeof(int64_t));
    if (!sizes) return 2;
    CK(hmsg_get_instance_sizes(h, sizes));
    printf("instances %ld\n", (long)N);
    for (i = 0; i < N; ++i) printf("size %ld\n", (long)sizes[i]);
    hmsg_destroy(h);
    return 0;
}
