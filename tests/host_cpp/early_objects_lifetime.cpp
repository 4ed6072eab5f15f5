// The object stage beside the pooling (hmsg_scene_graph.hip: EarlyObjects) driven from a plain C++ program: begin -> pool -> finish
// with the stage on and off, and the order / lifetime cases of tests/test_graph_early_objects.py -- a graph closed before the
// pooling, a reset between pool and finish followed by a second build, a scene destroyed without a finish, two scenes built by two
// threads at once.  Linked against the kernel simulator's objects it is what scripts/early_objects_sanitize.sh runs under the
// host's AddressSanitizer (the worker thread, its stream, the allocator cache it borrows and the hand-over of its buffers are all
// host code).  Input: the file tests/test_c_host.py writes for tests/host_c/hmsg_host.c (its head is read here).
//   early_objects_lifetime <in.bin>      prints "early objects: ok" and returns 0
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "hmsg_test.h"

namespace {

struct In {
    int32_t F, H, W, M, D, nb, dbmin;
    double radius;
    std::vector<double> K, pose;
    std::vector<uint8_t> rgb, masks;
    std::vector<uint16_t> depth;
    std::vector<int32_t> n_masks;
    std::vector<float> f_g, f_masked, f_crop;
};

template <typename T>
bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return fread(v.data(), sizeof(T), n, f) == n;
}

[[noreturn]] void die(const std::string& what) {
    fprintf(stderr, "early_objects_lifetime: %s\n", what.c_str());
    exit(3);
}
void ck(int rc, hmsg_t* h, const char* what) {
    if (rc != HMSG_OK) die(std::string(what) + ": " + (h ? hmsg_last_error(h) : "?"));
}
void ckg(int rc, hmsg_graph_t* g, const char* what) {
    if (rc != HMSG_OK) die(std::string(what) + ": " + hmsg_graph_last_error(g));
}
int state(const hmsg_graph_t* g, const hmsg_t* h) {
    int32_t st = -1, live = -1;
    if (hmsg_test_graph_early_objects(g, h, &st, &live) != HMSG_OK) die("hook");
    return st;
}
int live_threads(const hmsg_t* h) {
    int32_t st = -1, live = -1;
    if (hmsg_test_graph_early_objects(nullptr, h, &st, &live) != HMSG_OK) die("hook");
    return live;
}

hmsg_t* scene(const In& in) {
    hmsg_config cfg;
    hmsg_default_config(&cfg);
    cfg.device_id = 0;
    cfg.feat_dim = in.D;
    cfg.height = in.H;
    cfg.width = in.W;
    cfg.max_frames = in.F;
    cfg.max_masks = in.M;
    cfg.outlier_radius = in.radius;
    cfg.outlier_nb_points = in.nb;
    cfg.feat_dbscan_min = in.dbmin;
    hmsg_t* h = nullptr;
    if (hmsg_create(&cfg, &h) != HMSG_OK || !h) die("hmsg_create");
    return h;
}
void map(const In& in, hmsg_t* h) {
    ck(hmsg_add_frames(h, in.F, in.rgb.data(), in.depth.data(), in.pose.data(), in.K.data()), h, "hmsg_add_frames");
    ck(hmsg_finalize_map(h), h, "hmsg_finalize_map");
}
hmsg_graph_t* begin(const In& in, hmsg_t* h) {
    hmsg_graph_params p;
    hmsg_graph_default_params(&p);
    p.num_views = 5;
    p.host_threads = 2;
    hmsg_graph_t* g = nullptr;
    ck(hmsg_graph_begin(h, &p, in.F, in.pose.data(), nullptr, in.f_g.data(), nullptr, &g), h, "hmsg_graph_begin");
    return g;
}
void to_pool(const In& in, hmsg_t* h) {
    ck(hmsg_add_frame_features(h, 0, in.F, in.M, in.masks.data(), in.f_g.data(), in.f_masked.data(), in.f_crop.data(), in.n_masks.data()), h,
       "hmsg_add_frame_features");
    ck(hmsg_fuse_frames(h), h, "hmsg_fuse_frames");
    ck(hmsg_merge_instances(h), h, "hmsg_merge_instances");
    ck(hmsg_pool_instances(h), h, "hmsg_pool_instances");
}
// what the build left: instance sizes and points, object records
struct Result {
    std::vector<int64_t> sizes;
    std::vector<double> pts;
    std::vector<hmsg_graph_object> objects;
    bool operator==(const Result& o) const {
        return sizes == o.sizes && pts == o.pts && objects.size() == o.objects.size() &&
               (objects.empty() || memcmp(objects.data(), o.objects.data(), objects.size() * sizeof(hmsg_graph_object)) == 0);
    }
};
void instances(hmsg_t* h, Result& r) {
    const int64_t N = hmsg_num_instances(h);
    r.sizes.assign((size_t)(N > 0 ? N : 0), 0);
    if (N > 0) ck(hmsg_get_instance_sizes(h, r.sizes.data()), h, "hmsg_get_instance_sizes");
    int64_t total = 0;
    for (int64_t s : r.sizes) total += s;
    r.pts.assign((size_t)total * 3, 0.0);
    if (total) ck(hmsg_get_instance_points(h, r.pts.data()), h, "hmsg_get_instance_points");
}
Result finish(hmsg_t* h, hmsg_graph_t* g) {
    ckg(hmsg_graph_finish(g, 0, nullptr, nullptr), g, "hmsg_graph_finish");
    Result r;
    instances(h, r);
    hmsg_graph_counts c;
    ckg(hmsg_graph_get_counts(g, &c), g, "hmsg_graph_get_counts");
    r.objects.resize((size_t)c.objects);
    if (c.objects) ckg(hmsg_graph_get_objects(g, r.objects.data(), c.objects), g, "hmsg_graph_get_objects");
    return r;
}
// one whole build; `mid`: the instances a caller reads between pool and finish
Result build(const In& in, int want_state, Result* mid = nullptr) {
    hmsg_t* h = scene(in);
    map(in, h);
    hmsg_graph_t* g = begin(in, h);
    to_pool(in, h);
    if (mid) instances(h, *mid);
    Result r = finish(h, g);
    if (state(g, nullptr) != want_state) die("a build ended in state " + std::to_string(state(g, nullptr)) + ", expected " + std::to_string(want_state));
    hmsg_graph_destroy(g);
    hmsg_destroy(h);
    return r;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: early_objects_lifetime <in.bin>\n");
        return 1;
    }
    In in;
    {
        FILE* f = fopen(argv[1], "rb");
        int32_t hd[10];
        if (!f || fread(hd, 4, 10, f) != 10) die("cannot read the input file");
        in.F = hd[0], in.H = hd[1], in.W = hd[2], in.M = hd[3], in.D = hd[4], in.nb = hd[7], in.dbmin = hd[8], in.radius = hd[9] / 1000.0;
        const size_t HW = (size_t)in.H * in.W, F = (size_t)in.F, M = (size_t)in.M, D = (size_t)in.D;
        if (!(rd(f, in.K, 9) && rd(f, in.rgb, F * HW * 3) && rd(f, in.depth, F * HW) && rd(f, in.pose, F * 16) && rd(f, in.masks, F * M * HW) &&
              rd(f, in.n_masks, F) && rd(f, in.f_g, F * D) && rd(f, in.f_masked, F * M * D) && rd(f, in.f_crop, F * M * D)))
            die("the input file is short");
        fclose(f);
    }
    // the serial path, then the stage beside the pooling: equal, and the handle between the calls is the serial path's
    setenv("HMSG_GRAPH_EARLY_OBJECTS", "0", 1);
    Result mid0, mid1;
    const Result ref = build(in, 0, &mid0);
    unsetenv("HMSG_GRAPH_EARLY_OBJECTS");
    if (ref.objects.empty() || mid0 == ref) die("the scene has no objects, or its per-object DBSCAN changes nothing");
    if (!(build(in, 1, &mid1) == ref) || !(mid1.sizes == mid0.sizes && mid1.pts == mid0.pts)) die("the stage beside the pooling gives another result");
    // a graph closed between begin and pool
    {
        hmsg_t* h = scene(in);
        map(in, h);
        hmsg_graph_destroy(begin(in, h));
        if (state(nullptr, h) != 2) die("closed graph: not discarded");
        to_pool(in, h);
        hmsg_graph_t* g = begin(in, h);
        if (!(finish(h, g) == ref) || state(g, nullptr) != 0) die("closed graph: the later graph differs");
        hmsg_graph_destroy(g);
        hmsg_destroy(h);
    }
    // reset between pool and finish, then a second build on the handle
    {
        hmsg_t* h = scene(in);
        map(in, h);
        hmsg_graph_t* g = begin(in, h);
        to_pool(in, h);
        if (state(g, nullptr) != 3) die("reset: no result was pending");
        ck(hmsg_reset(h), h, "hmsg_reset");
        if (state(g, nullptr) != 2) die("reset: not discarded");
        hmsg_graph_destroy(g);
        map(in, h);
        g = begin(in, h);
        to_pool(in, h);
        if (!(finish(h, g) == ref) || state(g, nullptr) != 1) die("reset: the second build differs");
        hmsg_graph_destroy(g);
        hmsg_destroy(h);
    }
    // pool, then destroy: the graph outlives its scene
    {
        hmsg_t* h = scene(in);
        map(in, h);
        hmsg_graph_t* g = begin(in, h);
        to_pool(in, h);
        hmsg_destroy(h);
        if (state(g, nullptr) != 2) die("destroy: not discarded");
        hmsg_graph_destroy(g);
    }
    // two scenes from two threads
    {
        Result out[2];
        std::thread a([&] { out[0] = build(in, 1); }), b([&] { out[1] = build(in, 1); });
        a.join();
        b.join();
        if (!(out[0] == ref) || !(out[1] == ref)) die("two threads: a build differs");
    }
    {
        hmsg_t* h = scene(in);
        if (live_threads(h) != 0) die("a thread of the stage was left behind");
        hmsg_destroy(h);
    }
    hmsg_release_cached_memory();
    printf("early objects: ok\n");
    return 0;
}
