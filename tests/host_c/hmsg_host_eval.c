/* A saved graph against ground truth from C through include/hmsg.h alone: hmsg_load -> hmsg_graph_evaluate (the reference's
 * HM3DSemanticEvaluator.evaluate_floors / evaluate_rooms / evaluate_objects on a graph read by load_hmsg_graph).
 * usage: hmsg_host_eval <graph dir> <gt.bin> <out.bin>
 *   gt.bin : int32 n_floors, n_rooms, n_objects, n_classes, D, n_top_k, eval_metric, 0; int64 n_room_pts, n_obj_pts;
 *            f64 floor_lower [n_floors], floor_upper [n_floors];
 *            f64 room_pts [n_room_pts][3]; int64 room_off [n_rooms + 1]; f64 room_min_h, room_max_h, room_mean_h [n_rooms];
 *            f64 obj_pts [n_obj_pts][3]; int64 obj_off [n_objects + 1]; f64 obb_center [n_objects][3], obb_dims [n_objects][3];
 *            int32 obj_name_id [n_objects]; f32 text_feats [n_classes][D]; int32 class_name_id [n_classes]; int32 top_k [n_top_k]
 *   out.bin: f64 [26 + n_top_k]: floors tp tn fp fn acc prec recall | rooms acc50 ap prec50 recall50 gt pred hydra_prec hydra_recall |
 *            objects ap gt pred | iou50 tp fp fn acc prec recall | top_k_auc assigned | top_k_acc [n_top_k] */
#include <stdio.h>
#include <stdlib.h>

#include "hmsg.h"

static int fail(const char* what, int rc, const hmsg_graph_t* g) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, g ? hmsg_graph_last_error(g) : "");
    return 1;
}

static void* take(FILE* f, size_t size, size_t n) {
    void* p = malloc(size * (n > 0 ? n : 1));
    if (!p || fread(p, size, n, f) != n) {
        fprintf(stderr, "gt.bin is short\n");
        exit(2);
    }
    return p;
}

int main(int argc, char** argv) {
    FILE* f;
    int32_t hdr[8];
    int64_t npts[2];
    hmsg_eval_gt gt;
    hmsg_eval_params prm;
    hmsg_eval_metrics m;
    hmsg_graph_t* g = NULL;
    int32_t* top_k;
    double *acc, out[26];
    int rc;
    if (argc != 4) {
        fprintf(stderr, "usage: %s <graph dir> <gt.bin> <out.bin>\n", argv[0]);
        return 2;
    }
    f = fopen(argv[2], "rb");
    if (!f || fread(hdr, 4, 8, f) != 8 || fread(npts, 8, 2, f) != 2) return 2;
    gt.n_floors = hdr[0], gt.n_rooms = hdr[1], gt.n_objects = hdr[2], gt.n_classes = hdr[3], gt.feat_dim = hdr[4];
    gt.floor_lower = (const double*)take(f, 8, (size_t)gt.n_floors);
    gt.floor_upper = (const double*)take(f, 8, (size_t)gt.n_floors);
    gt.room_pts = (const double*)take(f, 8, (size_t)npts[0] * 3);
    gt.room_off = (const int64_t*)take(f, 8, (size_t)gt.n_rooms + 1);
    gt.room_min_h = (const double*)take(f, 8, (size_t)gt.n_rooms);
    gt.room_max_h = (const double*)take(f, 8, (size_t)gt.n_rooms);
    gt.room_mean_h = (const double*)take(f, 8, (size_t)gt.n_rooms);
    gt.obj_pts = (const double*)take(f, 8, (size_t)npts[1] * 3);
    gt.obj_off = (const int64_t*)take(f, 8, (size_t)gt.n_objects + 1);
    gt.obj_obb_center = (const double*)take(f, 8, (size_t)gt.n_objects * 3);
    gt.obj_obb_dims = (const double*)take(f, 8, (size_t)gt.n_objects * 3);
    gt.obj_name_id = (const int32_t*)take(f, 4, (size_t)gt.n_objects);
    gt.text_feats = (const float*)take(f, 4, (size_t)gt.n_classes * (size_t)gt.feat_dim);
    gt.class_name_id = (const int32_t*)take(f, 4, (size_t)gt.n_classes);
    top_k = (int32_t*)take(f, 4, (size_t)hdr[5]);
    fclose(f);
    hmsg_eval_default_params(&prm);
    prm.eval_metric = hdr[6];
    prm.n_top_k = hdr[5];
    prm.top_k = top_k;
    acc = (double*)calloc((size_t)(hdr[5] > 0 ? hdr[5] : 1), 8);
    if ((rc = hmsg_load(argv[1], 0, &g)) != HMSG_OK) return fail("hmsg_load", rc, NULL);
    if ((rc = hmsg_graph_evaluate(g, &gt, &prm, &m, acc)) != HMSG_OK) return fail("hmsg_graph_evaluate", rc, g);
    out[0] = (double)m.floors.tp, out[1] = (double)m.floors.tn, out[2] = (double)m.floors.fp, out[3] = (double)m.floors.fn;
    out[4] = m.floors.acc, out[5] = m.floors.prec, out[6] = m.floors.recall;
    out[7] = m.room_acc50, out[8] = m.room_ap, out[9] = m.room_prec50, out[10] = m.room_recall50;
    out[11] = (double)m.room_gt, out[12] = (double)m.room_pred, out[13] = m.room_hydra_prec, out[14] = m.room_hydra_recall;
    out[15] = m.obj_ap, out[16] = (double)m.obj_gt, out[17] = (double)m.obj_pred;
    out[18] = (double)m.obj_iou50.tp, out[19] = (double)m.obj_iou50.fp, out[20] = (double)m.obj_iou50.fn;
    out[21] = m.obj_iou50.acc, out[22] = m.obj_iou50.prec, out[23] = m.obj_iou50.recall;
    out[24] = m.obj_top_k_auc, out[25] = (double)m.obj_assigned;
    f = fopen(argv[3], "wb");
    if (!f) return 2;
    fwrite(out, 8, 26, f);
    fwrite(acc, 8, (size_t)hdr[5], f);
    fclose(f);
    hmsg_graph_destroy(g);
    free(acc);
    free(top_k);
    printf("hmsg_host_eval ok: %d rooms, %d objects\n", (int)m.room_pred, (int)m.obj_pred);
    return 0;
}
