/* The semantic segmentation score from C through include/hmsg.h alone (the reference's utils/eval_utils.py + utils/metric.py on a
 * feature map: text_prompt, sim_2_label, knn_interpolation, mean_iou ...): a small scene is built as the other C hosts build one --
 * frames, map, encoder outputs, fusion, merge, pooling -- and scored against a labelled ground-truth cloud by ONE call,
 * hmsg_evaluate_semseg.
 *   hmsg_host_semseg <in.bin> <out.bin>
 *   in : i32 F H W M D C k L n_ignore outlier_nb feat_dbscan_min outlier_radius_mm | i64 m | f64 K[9] | u8 rgb[F][H][W][3] |
 *        u16 depth[F][H][W] | f64 pose[F][16] | u8 masks[F][M][H][W] | i32 n_masks[F] | f32 f_g[F][D] | f32 f_masked[F][M][D] |
 *        f32 f_crop[F][M][D] | f32 text[C][D] | i32 class_label[C] | f64 gt_pts[m][3] | i32 gt_label[m] | i32 ignore[n_ignore]
 *   out: f64 miou fmiou acc macc | f64 per_class_iou[L] | i64 conf[L][L]
 * and prints the four scores with 17 significant digits. */
#include <stdio.h>
#include <stdlib.h>

#include "hmsg.h"

static void* rd(FILE* f, size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (!p || (bytes && fread(p, 1, bytes, f) != bytes)) {
        fprintf(stderr, "hmsg_host_semseg: short read (%lu bytes)\n", (unsigned long)bytes);
        exit(2);
    }
    return p;
}

#define CK(call)                                                                                 \
    do {                                                                                         \
        int rc_ = (call);                                                                        \
        if (rc_ != HMSG_OK) {                                                                    \
            fprintf(stderr, "hmsg_host_semseg: %s -> %d: %s\n", #call, rc_, hmsg_last_error(h)); \
            return 3;                                                                            \
        }                                                                                        \
    } while (0)

int main(int argc, char** argv) {
    FILE *fi, *fo;
    int32_t hd[12], F, H, W, M, D, C, k, L, n_ignore;
    int64_t m;
    double *K, *pose, *gt_pts, *per_class, sc4[4];
    uint8_t *rgb, *masks;
    uint16_t* depth;
    int32_t *n_masks, *class_label, *gt_label, *ignore;
    float *f_g, *f_masked, *f_crop, *text;
    int64_t* conf;
    hmsg_config cfg;
    hmsg_t* h = NULL;
    hmsg_semseg_scores sc;
    size_t HW;

    if (argc != 3) {
        fprintf(stderr, "usage: hmsg_host_semseg <in.bin> <out.bin>   (%s)\n", hmsg_version());
        return 1;
    }
    fi = fopen(argv[1], "rb");
    if (!fi) return 1;
    if (fread(hd, 4, 12, fi) != 12 || fread(&m, 8, 1, fi) != 1) return 2;
    F = hd[0]; H = hd[1]; W = hd[2]; M = hd[3]; D = hd[4]; C = hd[5]; k = hd[6]; L = hd[7]; n_ignore = hd[8];
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
    text = (float*)rd(fi, (size_t)C * (size_t)D * 4);
    class_label = (int32_t*)rd(fi, (size_t)C * 4);
    gt_pts = (double*)rd(fi, (size_t)m * 3 * sizeof(double));
    gt_label = (int32_t*)rd(fi, (size_t)m * 4);
    ignore = (int32_t*)rd(fi, (size_t)n_ignore * 4);
    fclose(fi);

    hmsg_default_config(&cfg);
    cfg.device_id = 0;
    cfg.feat_dim = D;
    cfg.height = H;
    cfg.width = W;
    cfg.max_frames = F;
    cfg.max_masks = M;
    cfg.outlier_nb_points = hd[9];
    cfg.feat_dbscan_min = hd[10];
    cfg.outlier_radius = (double)hd[11] / 1000.0;
    if (hmsg_create(&cfg, &h) != HMSG_OK || !h) {
        fprintf(stderr, "hmsg_host_semseg: hmsg_create failed: %s\n", hmsg_last_error(NULL));
        return 4;
    }
    CK(hmsg_add_frames(h, F, rgb, depth, pose, K));
    CK(hmsg_finalize_map(h));
    CK(hmsg_add_frame_features(h, 0, F, M, masks, f_g, f_masked, f_crop, n_masks));
    CK(hmsg_fuse_frames(h));
    CK(hmsg_merge_instances(h));
    CK(hmsg_pool_instances(h));
    per_class = (double*)calloc((size_t)L, sizeof(double));
    conf = (int64_t*)calloc((size_t)L * (size_t)L, sizeof(int64_t));
    if (!per_class || !conf) return 5;
    CK(hmsg_evaluate_semseg(h, text, C, class_label, gt_pts, gt_label, m, k, L, n_ignore ? ignore : NULL, n_ignore, &sc, per_class, conf));
    sc4[0] = sc.miou; sc4[1] = sc.fmiou; sc4[2] = sc.acc; sc4[3] = sc.macc;
    fo = fopen(argv[2], "wb");
    if (!fo) return 1;
    fwrite(sc4, sizeof(double), 4, fo);
    fwrite(per_class, sizeof(double), (size_t)L, fo);
    fwrite(conf, sizeof(int64_t), (size_t)L * (size_t)L, fo);
    fclose(fo);
    printf("miou %.17g fmiou %.17g acc %.17g macc %.17g instances %ld\n", sc.miou, sc.fmiou, sc.acc, sc.macc, (long)hmsg_num_instances(h));
    hmsg_destroy(h);
    free(K); free(rgb); free(depth); free(pose); free(masks); free(n_masks); free(f_g); free(f_masked); free(f_crop);
    free(text); free(class_label); free(gt_pts); free(gt_label); free(ignore); free(per_class); free(conf);
    return 0;
}
