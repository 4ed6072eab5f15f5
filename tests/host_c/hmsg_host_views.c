/* The slow path of the query applications from C through include/hmsg.h alone (Graph.query_room_obj_slow_reasoning, graph.py:2578-3054,
 * without its VLM calls -- the "VLM" here always picks the CLIP goal image):
 *   hmsg_load -> hmsg_graph_query (fast path, top 1) -> hmsg_graph_object_best_views -> hmsg_graph_goal_views ->
 *   hmsg_graph_find_view of the goal image -> hmsg_graph_rematch_in_views with the distance -> hmsg_graph_object_view_depths of the
 *   original hit in its own best view.
 * usage: hmsg_host_views <graph dir> <in.bin> <out.bin>
 *   in.bin : int32 D, Q, k, W, H, F; f32 T [Q][D]; f64 K [9]; f64 pose_inv [F][16] (world -> camera of image id i)
 *   out.bin: int32 hit [Q], best_view [Q]; int64 best_img [Q]; int32 n_goal [Q]; int64 goal_img [Q][k]; int32 goal_room [Q][k];
 *            f64 goal_score [Q][k]; int32 goal_view [Q], rematch [Q]; f64 rematch_score [Q], avg_distance [Q]; uint8 visible [Q];
 *            f64 mean_depth [Q]   (a query without a best view / goal view keeps -1 / 0 there) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hmsg.h"

static int fail(const char* what, int rc, const hmsg_graph_t* g) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, g ? hmsg_graph_last_error(g) : "");
    return 1;
}

static int read_all(FILE* f, void* p, size_t size, size_t n) { return fread(p, size, n, f) == n; }

int main(int argc, char** argv) {
    FILE* fi;
    FILE* fo;
    int32_t hdr[6], D, Q, k, W, H, F, RM, q, n;
    float* T;
    double K[9], *pose_inv, *score, *goal_score, *re_score, *avg, *cam, *md;
    int32_t *qid, *floor_id, *mode, *sel, *nsel, *hit, *room, *best_view, *n_goal, *goal_room, *goal_view, *rematch, *wh, *sub, *sub_view;
    int64_t *best_img, *goal_img;
    uint8_t* vis;
    hmsg_graph_t* g = NULL;
    hmsg_graph_counts cnt;
    int rc;
    if (argc != 4) {
        fprintf(stderr, "usage: %s <graph dir> <in.bin> <out.bin>\n", argv[0]);
        return 2;
    }
    fi = fopen(argv[2], "rb");
    if (!fi || !read_all(fi, hdr, 4, 6)) return 2;
    D = hdr[0], Q = hdr[1], k = hdr[2], W = hdr[3], H = hdr[4], F = hdr[5];
    T = (float*)malloc((size_t)Q * D * 4);
    pose_inv = (double*)malloc((size_t)F * 16 * 8);
    if (!read_all(fi, T, 4, (size_t)Q * D) || !read_all(fi, K, 8, 9) || !read_all(fi, pose_inv, 8, (size_t)F * 16)) return 2;
    fclose(fi);
    if ((rc = hmsg_load(argv[1], 0, &g)) != HMSG_OK) return fail("hmsg_load", rc, NULL);
    if ((rc = hmsg_graph_get_counts(g, &cnt)) != HMSG_OK) return fail("hmsg_graph_get_counts", rc, g);
    RM = cnt.rooms > 10 ? cnt.rooms : 10;
    /* 1. the fast path: every room, top 1 */
    qid = (int32_t*)calloc((size_t)Q, 4);
    mode = (int32_t*)calloc((size_t)Q, 4);
    floor_id = (int32_t*)malloc((size_t)Q * 4);
    for (q = 0; q < Q; ++q) floor_id[q] = -1;
    sel = (int32_t*)malloc((size_t)Q * RM * 4);
    nsel = (int32_t*)malloc((size_t)Q * 4);
    hit = (int32_t*)malloc((size_t)Q * 4);
    room = (int32_t*)malloc((size_t)Q * 4);
    score = (double*)malloc((size_t)Q * 8);
    rc = hmsg_graph_query(g, NULL, Q, 1, T, qid, NULL, floor_id, mode, 1, 0, RM, sel, nsel, hit, room, score);
    if (rc != HMSG_OK) return fail("hmsg_graph_query", rc, g);
    /* 2. best view of the hit (graph.py:2759-2765, :2828-2831) */
    best_view = (int32_t*)malloc((size_t)Q * 4);
    best_img = (int64_t*)malloc((size_t)Q * 8);
    if ((rc = hmsg_graph_object_best_views(g, Q, hit, best_view, best_img)) != HMSG_OK) return fail("hmsg_graph_object_best_views", rc, g);
    /* 3. goal images by CLIP (:2864-2897) */
    n_goal = (int32_t*)malloc((size_t)Q * 4);
    goal_img = (int64_t*)malloc((size_t)Q * k * 8);
    goal_room = (int32_t*)malloc((size_t)Q * k * 4);
    goal_score = (double*)malloc((size_t)Q * k * 8);
    if ((rc = hmsg_graph_goal_views(g, Q, T, floor_id, k, goal_img, goal_room, goal_score, n_goal)) != HMSG_OK) return fail("hmsg_graph_goal_views", rc, g);
    /* 4. the view of the chosen image (find_view_by_imgpath, :2965) and the re-match in it (:2968-2996) */
    goal_view = (int32_t*)malloc((size_t)Q * 4);
    rematch = (int32_t*)malloc((size_t)Q * 4);
    re_score = (double*)calloc((size_t)Q, 8);
    avg = (double*)calloc((size_t)Q, 8);
    sub = (int32_t*)malloc((size_t)Q * 4);
    sub_view = (int32_t*)malloc((size_t)Q * 4);
    cam = (double*)malloc((size_t)Q * 16 * 8);
    wh = (int32_t*)malloc((size_t)Q * 2 * 4);
    for (q = 0; q < Q; ++q) wh[2 * q] = W, wh[2 * q + 1] = H;
    for (q = 0; q < Q; ++q) {
        goal_view[q] = rematch[q] = -1;
        if (n_goal[q] > 0 && (rc = hmsg_graph_find_view(g, NULL, goal_img[(size_t)q * k], &goal_view[q])) != HMSG_OK) return fail("hmsg_graph_find_view", rc, g);
    }
    for (q = 0; q < Q; ++q) {            /* one query at a time, as the reference does; the call takes batches as well */
        double s = 0.0, a = 0.0;
        int64_t img;
        if (goal_view[q] < 0) continue;
        img = goal_img[(size_t)q * k];
        if (img < 0 || img >= F) return 2;
        rc = hmsg_graph_rematch_in_views(g, 1, T + (size_t)q * D, &goal_view[q], pose_inv + (size_t)img * 16, wh, K, &rematch[q], &s, &a);
        if (rc != HMSG_OK) return fail("hmsg_graph_rematch_in_views", rc, g);
        re_score[q] = s;
        avg[q] = a;
    }
    /* 5. the original hit in its own best view (:3011-3022) */
    vis = (uint8_t*)calloc((size_t)Q, 1);
    md = (double*)calloc((size_t)Q, 8);
    n = 0;
    for (q = 0; q < Q; ++q)
        if (best_view[q] >= 0 && best_img[q] >= 0 && best_img[q] < F) {
            sub[n] = hit[q];
            sub_view[n] = q;
            memcpy(cam + (size_t)n * 16, pose_inv + (size_t)best_img[q] * 16, 128);
            ++n;
        }
    if (n > 0) {
        uint8_t* v = (uint8_t*)malloc((size_t)n);
        double* m = (double*)malloc((size_t)n * 8);
        if ((rc = hmsg_graph_object_view_depths(g, n, sub, cam, wh, K, v, m)) != HMSG_OK) return fail("hmsg_graph_object_view_depths", rc, g);
        for (q = 0; q < n; ++q) vis[sub_view[q]] = v[q], md[sub_view[q]] = m[q];
        free(v), free(m);
    }
    for (q = 0; q < Q; ++q)
        printf("query %d: hit %d, best view %d (image %lld), goal image %lld (view %d), re-match %d score %.17g at %.17g m, online depth %.17g (%s)\n", (int)q,
               (int)hit[q], (int)best_view[q], (long long)best_img[q], (long long)(n_goal[q] > 0 ? goal_img[(size_t)q * k] : -1), (int)goal_view[q],
               (int)rematch[q], re_score[q], avg[q], md[q], vis[q] ? "visible" : "not visible");
    fo = fopen(argv[3], "wb");
    if (!fo) return 2;
    fwrite(hit, 4, (size_t)Q, fo);
    fwrite(best_view, 4, (size_t)Q, fo);
    fwrite(best_img, 8, (size_t)Q, fo);
    fwrite(n_goal, 4, (size_t)Q, fo);
    fwrite(goal_img, 8, (size_t)Q * k, fo);
    fwrite(goal_room, 4, (size_t)Q * k, fo);
    fwrite(goal_score, 8, (size_t)Q * k, fo);
    fwrite(goal_view, 4, (size_t)Q, fo);
    fwrite(rematch, 4, (size_t)Q, fo);
    fwrite(re_score, 8, (size_t)Q, fo);
    fwrite(avg, 8, (size_t)Q, fo);
    fwrite(vis, 1, (size_t)Q, fo);
    fwrite(md, 8, (size_t)Q, fo);
    fclose(fo);
    hmsg_graph_destroy(g);
    free(T), free(pose_inv), free(qid), free(mode), free(floor_id), free(sel), free(nsel), free(hit), free(room), free(score), free(best_view);
    free(best_img), free(n_goal), free(goal_img), free(goal_room), free(goal_score), free(goal_view), free(rematch), free(re_score), free(avg);
    free(sub), free(sub_view), free(cam), free(wh), free(vis), free(md);
    printf("hmsg_host_views ok: %d queries\n", (int)Q);
    return 0;
}
