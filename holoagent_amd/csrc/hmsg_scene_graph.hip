// The graph as ONE object behind the boundary (hmsg_build_graph, hmsg_save / hmsg_load of the whole directory):
//   build_hier_multimodal_scene_graph (graph.py:2033-2076) = segment_floors_manually (:624-787) -> per storey segment_hmsg_room
//   (:920-1189: regions, room clouds, compute_room_embeddings utils/graph_utils.py:192-356, Room and View nodes) ->
//   segment_hmsg_objects (:1582-1736) -> create_graph_new (:1752-1775); save_hmsg_graph (:1801-1824); load_hmsg_graph (:1892-1987).
// Every stage is a call that already exists in this library (hmsg_segment_floors / _rooms, hmsg_room_clouds,
// hmsg_room_camera_distances, hmsg_assign_cameras_to_rooms, hmsg_kmeans, hmsg_pick_representative_views,
// hmsg_build_object_nodes, hmsg_object_views, hmsg_graph_edges, hmsg_write_json / _ply, hmsg_save_objects); what the Python
// mirror holoagent_amd/graph.py did between them -- ids, names, lists, the bookkeeping of views and objects -- is host C++ here,
// so a C / C++ host builds, saves, loads and queries with four calls (tests/host_c/hmsg_host.c) and the benchmark's graph
// assembly is no longer Python.  The KMeans fits of a storey's rooms run on host threads (or, hmsg_graph_params::kmeans_device,
// as one batch per storey on the device) between hmsg_graph_begin (right after hmsg_finalize_map) and hmsg_graph_finish (after
// hmsg_pool_instances): beside the fusion and the merge fold.
#include "hmsg_boundary.h"
#include "hmsg_dbscan.h"
#include "hmsg_query.h"
#include "hmsg_query_views.h"
#include "hmsg_stage_files.h"

#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <mutex>
#include <thread>
#include <vector>

namespace {

struct GFloor {
    std::string id, name;
    hmsg_floor f{};
    double verts[8][3] = {};
    bool have_verts = false;
    std::vector<int> rooms;                 // global room indices, in floors[f].rooms order
    std::vector<double> pts;                // loaded graphs: the cloud read back (built graphs: the map's slab, fetched on save)
};
struct GRoom {
    std::string id, name;
    int floor = 0, index_in_floor = 0;
    std::vector<double> verts;              // [n][2] (x, z)
    double zero = 0, height = 0;
    bool have_level = false;
    std::vector<int> sel;                   // built: indices into the storey's floor cloud (hmsg_room_clouds)
    std::vector<double> pts;                // loaded: the cloud
    std::vector<float> emb;                 // [n_emb][D] room.embeddings (representative views)
    int n_emb = 0;
    std::vector<double> emb64;              // loaded: the same as json.load gives them
    std::vector<long long> represent, sample;
    std::vector<float> clip;                // [n_clip][D] room.clip_embeddings
    int n_clip = 0;
    std::vector<int> objects, views;        // global indices
    std::vector<std::string> view_ids;      // loaded graphs keep the ids as the record has them
    // the room level in flight (hmsg_graph_begin): rows to cluster
    std::vector<int> imgs;                  // view (processed-frame) indices assigned to the room
    std::vector<int> km_labels;
    std::vector<float> km_centers;
};
struct GView {
    std::string id;
    int floor = 0, room_in_floor = 0;       // the reference's View.room_id of a freshly built graph: the per-floor room INDEX (:1176-1189)
    std::string room_id_str;                // loaded graphs: "f_r"
    long long img = 0;
    bool have_img = true;
    std::string img_path;
    bool have_path = false;
    std::vector<int> objects;               // global object indices, ascending
    std::vector<std::string> object_ids, texts;
};
struct GObject {
    std::string id, name, room_id;
    int room = 0, instance = -1, label = -1, counter = 0;
    std::vector<int> views;                 // global view indices, in pair order
    std::vector<std::string> view_ids;
    int best_view = -1;
    std::string best_view_id;
    bool have_best = false;
    std::vector<double> emb;                // loaded: float64 embedding
    std::vector<double> pts;                // loaded
    std::vector<double> verts;              // loaded [n][2]
    // Room.merge_objects (hmsg_graph_params::merge_objects_graph): the instances whose clouds make up the object's cloud, in the
    // order Object.__add__ concatenated them (one: the object as segment_hmsg_objects made it), and its float32 embedding
    // (the mean chain of object.py:102); filled for every object once a graph has merged
    std::vector<int> parts;
    std::vector<float> emb32;
};

// What the object stage makes without the pooled features (graph.py:1582-1736 minus the labels): the View nodes, the per-object
// DBSCAN as a value of its own, object nodes with label -1, and the view <-> object test of every (object, view of its room) pair.
// hmsg_graph_finish takes it over -- from the early stage that ran beside the pooling, or from its own run of the same steps.
struct ObjStage {
    std::vector<GView> views;
    std::vector<std::vector<int>> room_views;   // per room: its views (global indices)
    InstanceSet den;                            // the denoised instances, not yet in the handle
    bool have_den = false;                      // false: the handle's list is the denoised one already (or there is nothing to denoise)
    std::vector<hmsg_node> nodes;               // label -1
    std::vector<int32_t> pair_inst, pair_view;
    std::vector<int> pair_obj;
    std::vector<uint8_t> vis;
    std::vector<double> md;
};
// the stage beside the pooling: a host thread and a stream of its own (hmsg_pool_instances starts and joins it)
struct EarlyObjects {
    std::thread th;
    bool ok = false;                            // ran to the end: `st` is complete
    unsigned long long epoch = 0;               // hmsg_ctx::inst_epoch it was made from
    double run_ms = 0;
    ObjStage st;
};

}  // namespace

struct hmsg_shard_ws;                       // (hmsg_query_sharded.hip)
void hmsg_shard_ws_free(hmsg_shard_ws* w);

struct hmsg_graph {
    hmsg_ctx* h = nullptr;                  // built graphs: the scene (object clouds and features stay in HBM); NULL after hmsg_load
    int device = 0, D = 0;
    hmsg_graph_params prm{};
    std::string err;
    std::vector<GFloor> floors;
    std::vector<GRoom> rooms;
    std::vector<GView> views;
    std::vector<GObject> objects;
    std::vector<long long> edges;           // pairs
    // inputs of the view level (copies: the caller's arrays may go away between begin and finish)
    int n_frames = 0;
    std::vector<double> poses, poses_inv;
    std::vector<float> feats;
    std::vector<std::string> img_paths;
    bool have_inv = false;
    std::vector<std::thread> workers;
    std::string worker_err;                 // first error of a KMeans worker (under worker_mu)
    std::mutex worker_mu;
    bool begun = false, finished = false, loaded = false;
    bool merged = false;                    // Room.merge_objects has run: objects carry parts / emb32, the index comes from them
    bool failed = false;                    // hmsg_graph_finish threw half way: views / objects are partly appended -- the graph only accepts hmsg_graph_destroy
    double t_begin_ms = 0, t_finish_ms = 0, t_kmeans_wait_ms = 0;
    hmsg_index_t* ix = nullptr;             // hmsg_graph_query's index (made on first use)
    hmsg_index_t* shard_ix = nullptr;       // the graph as a shard of hmsg_graph_query_sharded / hmsg_graphs_query: its own index, made
                                            // without room names (they come with every call); the levels above the nodes only for a
                                            // graph without objects.  hmsg_graph_query's `ix` is never touched by that path.
    hmsg_shard_ws* shard_ws = nullptr;      // that path's scratch, kept between calls (hmsg_query_sharded.hip)
    // the view level of the slow path (hmsg_graph_goal_views, hmsg_graph_rematch_in_views, hmsg_graph_object_view_depths), each made on
    // first use and freed with the graph
    hmsg_goal_table* goal = nullptr;        // every sampled image's CLIP embedding, float64 in HBM
    std::vector<std::string> goal_bad;      // per room: "" or why its rows cannot be searched (the reference asserts there, :2870)
    std::vector<std::vector<int>> view_lists;   // per view: find_object_by_object_id of every entry of object_ids, in that order; made
                                                // by hmsg_graph_finish / hmsg_load with the views, so the listing calls only read
    bool views_on_index = false;            // view_lists are resident on shard_ix (hmsg_index_set_views)
    DevBuf<double> obj_pts;                 // loaded graphs: the objects' clouds one after the other, uploaded once
    std::vector<long long> obj_pts_off;
    bool have_obj_pts = false;
    hipStream_t view_stream = nullptr;      // the stream of the distance kernels
    // the object stage beside the pooling: `registered` says that h->early_graph points here (the scene clears both when it goes first)
    bool registered = false;
    std::unique_ptr<EarlyObjects> early;
    int early_state = HMSG_EARLY_NEVER_MADE;
    double t_early_ms = 0, t_early_wait_ms = 0;
    ~hmsg_graph() {
        if (registered && h) hmsg_graph_early_abort(h);
        for (auto& t : workers)
            if (t.joinable()) t.join();
        if (ix) hmsg_index_destroy(ix);
        if (shard_ix) hmsg_index_destroy(shard_ix);
        if (shard_ws) hmsg_shard_ws_free(shard_ws);
        if (goal) hmsg_goal_table_free(goal);
        if (view_stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(view_stream);
            (void)hipStreamDestroy(view_stream);
        }
    }
};

namespace {

void need(int rc, hmsg_ctx* h, const char* what) {
    if (rc != HMSG_OK) throw hmsg_error{rc, std::string(what) + ": " + (h ? hmsg_last_error(h) : "failed")};
}

// json.dumps(str) (ensure_ascii=True)
std::string jstr(const std::string& s) {
    std::string o = "\"";
    char buf[16];
    for (size_t i = 0; i < s.size();) {
        const unsigned char c = (unsigned char)s[i];
        if (c == '"') o += "\\\"", ++i;
        else if (c == '\\') o += "\\\\", ++i;
        else if (c == '\n') o += "\\n", ++i;
        else if (c == '\r') o += "\\r", ++i;
        else if (c == '\t') o += "\\t", ++i;
        else if (c == '\b') o += "\\b", ++i;
        else if (c == '\f') o += "\\f", ++i;
        else if (c < 0x20) snprintf(buf, sizeof buf, "\\u%04x", c), o += buf, ++i;
        else if (c < 0x80) o += (char)c, ++i;
        else {                                        // UTF-8 -> \uXXXX (surrogate pair above the BMP)
            unsigned cp = 0;
            int n = c >= 0xf0 ? 4 : (c >= 0xe0 ? 3 : 2);
            cp = c & (n == 4 ? 0x07 : (n == 3 ? 0x0f : 0x1f));
            for (int k = 1; k < n && i + k < s.size(); ++k) cp = (cp << 6) | ((unsigned char)s[i + k] & 0x3f);
            i += (size_t)n;
            if (cp >= 0x10000) {
                cp -= 0x10000;
                snprintf(buf, sizeof buf, "\\u%04x\\u%04x", 0xd800 + (cp >> 10), 0xdc00 + (cp & 0x3ff));
            } else {
                snprintf(buf, sizeof buf, "\\u%04x", cp);
            }
            o += buf;
        }
    }
    return o + "\"";
}
std::string jlist(const std::vector<std::string>& v) {    // json.dumps(list of str)
    std::string o = "[";
    for (size_t i = 0; i < v.size(); ++i) {
        if (i) o += ", ";
        o += jstr(v[i]);
    }
    return o + "]";
}

// np.arange(start, stop, step): length ceil((stop - start) / step), value i = start + i * ((start + step) - start)
std::vector<double> np_arange(double start, double stop, double step) {
    const double len = std::ceil((stop - start) / step);
    const long long n = len > 0 ? (long long)len : 0;
    std::vector<double> v((size_t)n);
    const double delta = (start + step) - start;
    for (long long i = 0; i < n; ++i) v[(size_t)i] = i == 0 ? start : (i == 1 ? start + step : start + (double)i * delta);
    return v;
}

// np.linalg.inv of a 4x4 (LAPACK dgesv on the identity: LU with partial pivoting, then the two triangular solves per column).
// The sequence of operations is the unblocked algorithm's; a LAPACK build that blocks or recurses differently may differ in the
// last bit, which is why hmsg_graph_begin also takes the inverses from a caller that has numpy's.
void inv4(const double* A, double* out) {
    double a[4][4];
    int piv[4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) a[i][j] = A[i * 4 + j];
    for (int k = 0; k < 4; ++k) {
        int p = k;
        for (int i = k + 1; i < 4; ++i)
            if (std::fabs(a[i][k]) > std::fabs(a[p][k])) p = i;
        piv[k] = p;
        if (p != k)
            for (int j = 0; j < 4; ++j) std::swap(a[k][j], a[p][j]);
        if (a[k][k] != 0.0) {
            const double r = 1.0 / a[k][k];
            for (int i = k + 1; i < 4; ++i) a[i][k] *= r;
        }
        for (int j = k + 1; j < 4; ++j)
            for (int i = k + 1; i < 4; ++i) a[i][j] -= a[i][k] * a[k][j];
    }
    for (int c = 0; c < 4; ++c) {
        double b[4] = {0, 0, 0, 0};
        b[c] = 1.0;
        for (int k = 0; k < 4; ++k)
            if (piv[k] != k) std::swap(b[k], b[piv[k]]);
        for (int k = 0; k < 4; ++k)                       // L y = P b (unit diagonal), column oriented as dtrsm does
            for (int i = k + 1; i < 4; ++i) b[i] -= b[k] * a[i][k];
        for (int k = 3; k >= 0; --k) {                    // U x = y
            b[k] /= a[k][k];
            for (int i = 0; i < k; ++i) b[i] -= b[k] * a[i][k];
        }
        for (int i = 0; i < 4; ++i) out[i * 4 + c] = b[i];
    }
}

void floor_vertices(GFloor& fl) {                         // Open3D AABB corner order (floor.py / SURVEY 8c)
    if (fl.f.n_points <= 0) return;
    const double* mn = fl.f.bbox_min;
    const double* mx = fl.f.bbox_max;
    const double ex[3] = {mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]};
    const double v[8][3] = {{mn[0], mn[1], mn[2]},         {mn[0] + ex[0], mn[1], mn[2]},         {mn[0], mn[1] + ex[1], mn[2]},
                            {mn[0], mn[1], mn[2] + ex[2]}, {mx[0], mx[1], mx[2]},                 {mn[0], mn[1] + ex[1], mn[2] + ex[2]},
                            {mn[0] + ex[0], mn[1], mn[2] + ex[2]}, {mn[0] + ex[0], mn[1] + ex[1], mn[2]}};
    memcpy(fl.verts, v, sizeof v);
    fl.have_verts = true;
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- stage 1 of segment_hmsg_room for one storey (graph.py:942-1136 + graph_utils.py:244-291): regions, room clouds (resident),
// camera -> room table, image lists; the KMeans rows are left in GRoom::imgs for the worker threads
void room_level_prepare(hmsg_graph* g, int fi) {
    hmsg_ctx* h = g->h;
    GFloor& fl = g->floors[(size_t)fi];
    const double res = h->cfg.grid_resolution > 0 ? h->cfg.grid_resolution : 0.05;
    int rows = 0, cols = 0, nr = 0;
    double xz_min[2] = {0, 0};
    need(hmsg_segment_rooms(h, fl.f.y_lo, fl.f.y_hi, fl.f.zero_level, fl.f.height, res, nullptr, 0, &rows, &cols, &nr, xz_min), h, "hmsg_segment_rooms");
    std::vector<int> markers((size_t)rows * (size_t)cols);
    if (!markers.empty())
        need(hmsg_segment_rooms(h, fl.f.y_lo, fl.f.y_hi, fl.f.zero_level, fl.f.height, res, markers.data(), (int64_t)markers.size(), &rows, &cols, &nr, xz_min),
             h, "hmsg_segment_rooms");
    // map_grid_to_point_cloud (graph_utils.py:359-388) of every room's cells, in np.where order (rows, then columns)
    std::vector<std::vector<double>> region((size_t)nr);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const int m = markers[(size_t)r * cols + c];
            if (m >= 1 && m <= nr) {
                auto& v = region[(size_t)m - 1];
                v.push_back(((double)c - 10.5) * res + xz_min[0]);
                v.push_back(((double)r - 10.5) * res + xz_min[1]);
            }
        }
    const size_t room0 = g->rooms.size();
    for (int i = 0; i < nr; ++i) {
        GRoom rm;
        rm.id = fl.id + "_" + std::to_string(i);
        rm.name = "room_" + std::to_string(i);
        rm.floor = fi;
        rm.index_in_floor = i;
        rm.verts = region[(size_t)i];
        rm.zero = fl.f.zero_level;
        rm.height = fl.f.height;
        rm.have_level = true;
        fl.rooms.push_back((int)g->rooms.size());
        g->rooms.push_back(std::move(rm));
    }
    if (nr == 0) return;
    // room clouds (:1086-1108) on the device, resident for the distance table
    std::vector<double> z_levels = np_arange(fl.f.zero_level, fl.f.zero_level + fl.f.height, 0.05);
    for (auto& z : z_levels) z *= -1.0;
    // T1: Rotation.from_euler("x", 90, degrees=True).as_matrix() as scipy gives it (cos 90 deg comes out as 2^-52)
    const double e = 2.220446049250313e-16;
    const double T1[16] = {1, 0, 0, 0, 0, e, -1, 0, 0, 1, e, 0, 0, 0, 0, 1};
    std::vector<int64_t> off((size_t)nr + 1, 0);
    std::vector<double> xz;
    for (int i = 0; i < nr; ++i) {
        const auto& v = g->rooms[room0 + (size_t)i].verts;
        off[(size_t)i + 1] = off[(size_t)i] + (int64_t)(v.size() / 2);
        xz.insert(xz.end(), v.begin(), v.end());
    }
    std::vector<int64_t> sizes((size_t)nr, 0);
    int64_t nf = 0;
    // (ONE call: a room's cloud is a subset of the storey's floor cloud, so rooms x storey points bounds the index list -- asking
    //  for the sizes first would run the nearest-neighbour search twice, 9 ms each at configs[1])
    const int64_t cap = (int64_t)nr * std::max<int64_t>(fl.f.n_points, 1);
    std::vector<int32_t> sel((size_t)cap);
    need(hmsg_room_clouds(h, fl.f.y_lo, fl.f.y_hi, T1, (int32_t)z_levels.size(), z_levels.data(), nr, off.data(), xz.data(), sizes.data(), sel.data(), cap, &nf),
         h, "hmsg_room_clouds");
    {
        int64_t o = 0;
        for (int i = 0; i < nr; ++i) {
            g->rooms[room0 + (size_t)i].sel.assign(sel.begin() + o, sel.begin() + o + sizes[(size_t)i]);
            o += sizes[(size_t)i];
        }
    }
    // camera -> room (compute_room_embeddings :244-291)
    const int F = g->n_frames;
    std::vector<double> cam((size_t)F * 2), height((size_t)F), dist((size_t)F * (size_t)nr);
    for (int i = 0; i < F; ++i) {
        cam[(size_t)i * 2] = g->poses[(size_t)i * 16 + 3];
        cam[(size_t)i * 2 + 1] = g->poses[(size_t)i * 16 + 11];
        height[(size_t)i] = g->poses[(size_t)i * 16 + 7];
    }
    if (F) need(hmsg_room_camera_distances(h, nr, F, cam.data(), dist.data()), h, "hmsg_room_camera_distances");
    std::vector<int32_t> room_of((size_t)std::max(F, 1)), imgs((size_t)F + (size_t)nr);
    std::vector<int64_t> roff((size_t)nr + 1);
    // (the floor cloud's y bounds: the storey's box came back with hmsg_segment_floors)
    need(hmsg_assign_cameras_to_rooms(dist.data(), F, nr, height.data(), fl.f.bbox_min[1], fl.f.bbox_max[1], room_of.data(), roff.data(), imgs.data()), h,
         "hmsg_assign_cameras_to_rooms");
    for (int i = 0; i < nr; ++i) g->rooms[room0 + (size_t)i].imgs.assign(imgs.begin() + roff[(size_t)i], imgs.begin() + roff[(size_t)i + 1]);
}

// ---- stage 2: KMeans(num_views) over a room's image embeddings + the representative picks (:329-352).  The fit is hmsg_kmeans on a
// host thread per room, or -- hmsg_graph_params::kmeans_device -- one hmsg_kmeans_batch call per storey on the device (the same bits)
// the rows to cluster; false: fewer images than num_views, every image represents the room (:297-301) and the room is done
bool room_rows(hmsg_graph* g, GRoom& rm) {
    const int D = g->D, n = (int)rm.imgs.size(), nv = g->prm.num_views, skip = std::max(1, g->prm.skip_frames);
    rm.clip.resize((size_t)n * D);
    for (int i = 0; i < n; ++i) memcpy(&rm.clip[(size_t)i * D], &g->feats[(size_t)rm.imgs[(size_t)i] * D], (size_t)D * 4);
    rm.n_clip = n;
    rm.sample.clear();
    for (int v : rm.imgs) rm.sample.push_back((long long)v * skip);
    rm.represent.clear();
    if (n < nv) {
        rm.emb = rm.clip;
        rm.n_emb = n;
        for (int v : rm.imgs) rm.represent.push_back((long long)v * skip);
        return false;
    }
    rm.km_labels.resize((size_t)n);
    rm.km_centers.resize((size_t)nv * D);
    return true;
}
void room_pick(hmsg_graph* g, GRoom& rm) {
    const int D = g->D, n = (int)rm.imgs.size(), nv = g->prm.num_views, skip = std::max(1, g->prm.skip_frames);
    std::vector<int32_t> member((size_t)nv);
    int32_t nm = 0;
    if (hmsg_pick_representative_views(rm.clip.data(), n, D, rm.km_labels.data(), rm.km_centers.data(), nv, member.data(), &nm) != HMSG_OK)
        throw hmsg_error{HMSG_ERR_INVALID, "hmsg_pick_representative_views failed"};
    rm.emb.resize((size_t)nm * D);
    rm.n_emb = nm;
    for (int k = 0; k < nm; ++k) {
        memcpy(&rm.emb[(size_t)k * D], &rm.clip[(size_t)member[(size_t)k] * D], (size_t)D * 4);
        rm.represent.push_back((long long)rm.imgs[(size_t)member[(size_t)k]] * skip);
    }
}
void room_embed(hmsg_graph* g, GRoom& rm) {
    if (!room_rows(g, rm)) return;
    const int rc = hmsg_kmeans(rm.clip.data(), (int)rm.imgs.size(), g->D, g->prm.num_views, g->prm.kmeans_n_init, g->prm.kmeans_max_iter,
                               g->prm.kmeans_seed, rm.km_labels.data(), rm.km_centers.data(), nullptr, nullptr);
    if (rc != HMSG_OK) throw hmsg_error{rc, "hmsg_kmeans failed"};
    room_pick(g, rm);
}
// the rooms of one storey that have at least num_views images: one hmsg_kmeans_batch call
void storey_embed_device(hmsg_graph* g, const GFloor& fl) {
    const int D = g->D, nv = g->prm.num_views;
    std::vector<int> fit;
    std::vector<int64_t> off(1, 0);
    for (int r : fl.rooms)
        if (room_rows(g, g->rooms[(size_t)r])) {
            fit.push_back(r);
            off.push_back(off.back() + (int64_t)g->rooms[(size_t)r].imgs.size());
        }
    if (fit.empty()) return;
    std::vector<float> X((size_t)off.back() * D), centers(fit.size() * (size_t)nv * D);
    std::vector<int32_t> labels((size_t)off.back());
    for (size_t i = 0; i < fit.size(); ++i) memcpy(&X[(size_t)off[i] * D], g->rooms[(size_t)fit[i]].clip.data(), (size_t)(off[i + 1] - off[i]) * D * 4);
    const int rc = hmsg_kmeans_batch(g->device, (int32_t)fit.size(), off.data(), X.data(), D, nv, g->prm.kmeans_n_init, g->prm.kmeans_max_iter,
                                     g->prm.kmeans_seed, labels.data(), centers.data(), nullptr, nullptr);
    if (rc != HMSG_OK) throw hmsg_error{rc, "hmsg_kmeans_batch failed"};
    for (size_t i = 0; i < fit.size(); ++i) {
        GRoom& rm = g->rooms[(size_t)fit[i]];
        rm.km_labels.assign(labels.begin() + (ptrdiff_t)off[i], labels.begin() + (ptrdiff_t)off[i + 1]);
        rm.km_centers.assign(centers.begin() + (ptrdiff_t)(i * (size_t)nv * D), centers.begin() + (ptrdiff_t)((i + 1) * (size_t)nv * D));
        room_pick(g, rm);
    }
}

}  // namespace
// (hmsg_objmerge.hip) room.py:62-129 for the objects of one room: groups [key object, objects added to it ...] in the new list's order
void hmsg_merge_groups(hmsg_ctx* h, int n, const double* points, const long long* start, const int* count, const int* name_id,
                       double overlap_threshold, double radius, std::vector<int>& group_off, std::vector<int>& members);
namespace {

// graph.py:2053-2058: every room fuses its same-name objects whose clouds overlap (Room.merge_objects) and re-numbers them; the
// graph's object list becomes the rooms' lists one after the other; a view keeps the object ids it was given (text_discription
// too) and is linked to the objects that carry one of those ids NOW (create_graph_new, :1764-1773) -- as the Python mirror does.
void graph_merge_objects(hmsg_graph* g, const std::vector<float>& node_emb) {
    hmsg_ctx* h = g->h;
    const int D = g->D;
    for (size_t k = 0; k < g->objects.size(); ++k) {
        GObject& o = g->objects[k];
        o.parts.assign(1, o.instance);
        o.emb32.assign(node_emb.begin() + (ptrdiff_t)(k * (size_t)D), node_emb.begin() + (ptrdiff_t)((k + 1) * (size_t)D));
    }
    std::vector<GObject> out;
    for (auto& rm : g->rooms) {
        const int n = (int)rm.objects.size();
        std::vector<int> name_id((size_t)n), count((size_t)n);
        std::vector<long long> start((size_t)n);
        std::map<std::string, int> ids;
        for (int i = 0; i < n; ++i) {
            const GObject& o = g->objects[(size_t)rm.objects[(size_t)i]];
            name_id[(size_t)i] = ids.emplace(o.name, (int)ids.size()).first->second;
            start[(size_t)i] = h->inst.off[(size_t)o.instance];
            count[(size_t)i] = (int)(h->inst.off[(size_t)o.instance + 1] - h->inst.off[(size_t)o.instance]);
        }
        std::vector<int> goff, mem;
        if (n) hmsg_merge_groups(h, n, h->inst.pts.p, start.data(), count.data(), name_id.data(), 0.01, 0.1, goff, mem);
        std::vector<int> fresh;
        for (size_t gi = 0; gi + 1 < goff.size(); ++gi) {
            GObject& key = g->objects[(size_t)rm.objects[(size_t)mem[(size_t)goff[gi]]]];
            for (int q = goff[gi] + 1; q < goff[gi + 1]; ++q) {
                // Object.__add__ (object.py:93-103; an object of the graph never has an empty cloud): clouds concatenated, embedding
                // = np.mean([a, b], axis=0) of two float32 rows
                const GObject& other = g->objects[(size_t)rm.objects[(size_t)mem[(size_t)q]]];
                key.parts.insert(key.parts.end(), other.parts.begin(), other.parts.end());
                for (int d = 0; d < D; ++d) key.emb32[(size_t)d] = (key.emb32[(size_t)d] + other.emb32[(size_t)d]) / 2.0f;
            }
            key.id = rm.id + "_" + std::to_string(gi);
            key.counter = (int)gi;
            fresh.push_back((int)out.size());
            out.push_back(key);             // (a copy: a later group may add to an object that an earlier one absorbed, as the reference does)
        }
        rm.objects = fresh;
    }
    g->objects.swap(out);
    std::map<std::string, std::vector<int>> pos;
    for (size_t k = 0; k < g->objects.size(); ++k) pos[g->objects[k].id].push_back((int)k);
    for (auto& v : g->views) {
        std::vector<int> ks;
        for (auto& oid : v.object_ids) {
            auto it = pos.find(oid);
            if (it != pos.end()) ks.insert(ks.end(), it->second.begin(), it->second.end());
        }
        std::sort(ks.begin(), ks.end());
        ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
        v.objects = ks;
    }
    g->merged = true;
}

void join_workers(hmsg_graph* g) {
    const double t0 = now_ms();
    for (auto& t : g->workers)
        if (t.joinable()) t.join();
    g->workers.clear();
    g->t_kmeans_wait_ms += now_ms() - t0;
    // (the workers are joined: no lock needed; the error stays, so every later call reports it again)
    if (!g->worker_err.empty()) throw hmsg_error{HMSG_ERR_INVALID, g->worker_err};
}

// per view: find_object_by_object_id (graph.py:2572-2576: the first object that carries the id) of every entry of view.object_ids,
// in that order (:2968-2973; an id no object carries makes the reference assert -- it is left out here)
void build_view_lists(hmsg_graph* g) {
    std::map<std::string, int> obj_of_id;
    for (size_t k = 0; k < g->objects.size(); ++k) obj_of_id.emplace(g->objects[k].id, (int)k);
    g->view_lists.assign(g->views.size(), {});
    for (size_t v = 0; v < g->views.size(); ++v)
        for (auto& oid : g->views[v].object_ids) {
            auto it = obj_of_id.find(oid);
            if (it != obj_of_id.end()) g->view_lists[v].push_back(it->second);
        }
}

// ---- stage 3: View nodes (:1176-1189), objects (:1582-1736), edges (:1752-1775)
// views: per floor, rooms in order, the room's images in order; the running index counts across the floor's rooms
void make_views(const hmsg_graph* g, std::vector<GView>& views, std::vector<std::vector<int>>& room_views) {
    const int skip = std::max(1, g->prm.skip_frames);
    room_views.assign(g->rooms.size(), {});
    for (size_t fi = 0; fi < g->floors.size(); ++fi) {
        int view_index = 0;
        for (int ri : g->floors[fi].rooms) {
            const GRoom& rm = g->rooms[(size_t)ri];
            for (int img : rm.imgs) {
                GView v;
                v.id = g->floors[fi].id + "_" + std::to_string(rm.index_in_floor) + "_" + std::to_string(view_index++);
                v.floor = (int)fi;
                v.room_in_floor = rm.index_in_floor;
                v.img = (long long)img * skip;
                if (!g->img_paths.empty() && (size_t)img < g->img_paths.size()) {
                    v.img_path = g->img_paths[(size_t)img];
                    v.have_path = true;
                }
                room_views[(size_t)ri].push_back((int)views.size());
                views.push_back(std::move(v));
            }
        }
    }
}
// the floors and rooms as hmsg_build_object_nodes takes them
struct RoomTables {
    std::vector<double> fz, fh, verts;
    std::vector<int32_t> room_floor;
    std::vector<int64_t> voff;
};
void room_tables(const hmsg_graph* g, RoomTables& t) {
    t.voff.assign(1, 0);
    for (auto& fl : g->floors) t.fz.push_back(fl.f.zero_level), t.fh.push_back(fl.f.height);
    for (auto& rm : g->rooms) {
        t.room_floor.push_back(rm.floor);
        t.verts.insert(t.verts.end(), rm.verts.begin(), rm.verts.end());
        t.voff.push_back(t.voff.back() + (int64_t)(rm.verts.size() / 2));
    }
}
// the camera of every view: world -> camera matrix, image size
void view_cameras(const hmsg_graph* g, const hmsg_ctx* h, const std::vector<GView>& views, std::vector<double>& pinv, std::vector<int32_t>& wh) {
    const int skip = std::max(1, g->prm.skip_frames);
    const size_t NV = views.size();
    pinv.resize(NV * 16);
    wh.resize(NV * 2);
    const int W = g->prm.image_width > 0 ? g->prm.image_width : h->cfg.width, H = g->prm.image_height > 0 ? g->prm.image_height : h->cfg.height;
    for (size_t v = 0; v < NV; ++v) {
        const size_t fr = (size_t)(views[v].img / skip);
        if (g->have_inv) memcpy(&pinv[v * 16], &g->poses_inv[fr * 16], 128);
        else inv4(&g->poses[fr * 16], &pinv[v * 16]);
        wh[v * 2] = W;
        wh[v * 2 + 1] = H;
    }
}
// one GObject per node, in node order
void add_objects(hmsg_graph* g, const std::vector<hmsg_node>& nodes, int64_t N, int32_t n_labels, const char* const* label_names) {
    for (int64_t k = 0; k < N; ++k) {
        const hmsg_node& nd = nodes[(size_t)k];
        GObject o;
        GRoom& rm = g->rooms[(size_t)nd.room];
        o.room = nd.room;
        o.room_id = rm.id;
        o.instance = nd.instance;
        o.label = nd.label;
        o.counter = nd.counter;
        o.id = rm.id + "_" + std::to_string(nd.counter);
        o.name = (label_names && nd.label >= 0 && nd.label < n_labels && label_names[nd.label]) ? label_names[nd.label] : "object";
        rm.objects.push_back((int)g->objects.size());
        g->objects.push_back(std::move(o));
    }
}
// the visible pairs into the objects' view lists, their best views and the views' object lists
void link_views(hmsg_graph* g, const std::vector<int>& pair_obj, const std::vector<int32_t>& pair_view, const std::vector<uint8_t>& vis,
                const std::vector<double>& md) {
    std::vector<double> best_d(g->objects.size(), 0.0);
    for (size_t p = 0; p < pair_obj.size(); ++p) {
        if (!vis[p]) continue;
        GObject& o = g->objects[(size_t)pair_obj[p]];
        o.views.push_back(pair_view[p]);
        // best view = the first strictly smallest mean depth, scanning from inf (:1727-1731): a non-finite mean never wins
        if (md[p] < (o.best_view < 0 ? INFINITY : best_d[(size_t)pair_obj[p]])) {
            o.best_view = pair_view[p];
            best_d[(size_t)pair_obj[p]] = md[p];
        }
        g->views[(size_t)pair_view[p]].objects.push_back(pair_obj[p]);   // (pairs come in object order: ascending per view)
    }
}

// The part of the object stage that needs nothing of the pooling, on stream s against the handle's merged instances, which it only
// reads: neither the graph nor the handle is written (but for the stage's own scratch, h->early_ops), everything goes into `st`.
void object_stage(const hmsg_graph* g, hmsg_ctx* h, hipStream_t s, ObjStage& st) {
    DbgLaps laps("early objects", s);
    make_views(g, st.views, st.room_views);
    laps.lap("view nodes");
    RoomTables t;
    room_tables(g, t);
    st.have_den = !h->inst_denoised && hmsg_denoise_compute(s, h->inst, 0.05, 10, st.den, &h->early_ops);
    laps.lap("per-object DBSCAN");
    const InstanceSet& inst = st.have_den ? st.den : h->inst;
    const int N = (int)inst.off.size() - 1, R = (int)g->rooms.size();
    if (N > 0) {
        std::vector<double> share((size_t)N * std::max(R, 1), 0.0);
        if (R > 0) hmsg_room_share_on(s, inst, R, (const long long*)t.voff.data(), t.verts.data(), 0.2, share.data());
        laps.lap("room shares");
        hmsg_object_nodes_on(s, inst, (int)g->floors.size(), t.fz.data(), t.fh.data(), R, t.room_floor.data(), t.voff.data(), t.verts.data(), share.data(),
                             st.nodes);
        laps.lap("floors / rooms (host)");
    }
    // view <-> object topology (:1712-1734): every (object, view of its room) pair in object order; object k is node k
    for (size_t k = 0; k < st.nodes.size(); ++k)
        for (int v : st.room_views[(size_t)st.nodes[k].room]) {
            st.pair_obj.push_back((int)k);
            st.pair_inst.push_back(st.nodes[k].instance);
            st.pair_view.push_back(v);
        }
    if (!st.pair_obj.empty()) {
        std::vector<double> pinv;
        std::vector<int32_t> wh;
        view_cameras(g, h, st.views, pinv, wh);
        HMSG_REQUIRE(h->have_K, HMSG_ERR_INVALID, "hmsg_graph_finish: no camera intrinsics (hmsg_add_frames)");
        st.vis.resize(st.pair_obj.size());
        st.md.resize(st.pair_obj.size());
        hmsg_object_views_on(s, inst, (int32_t)st.views.size(), pinv.data(), wh.data(), h->K, (int64_t)st.pair_obj.size(), st.pair_inst.data(),
                             st.pair_view.data(), g->prm.min_visible_ratio, g->prm.max_view_depth, st.vis.data(), st.md.data());
        laps.lap("hmsg_object_views");
    }
}

std::atomic<int> g_early_threads{0};        // early-stage threads started and not yet joined (test hook)

void early_drop(hmsg_graph* g, hmsg_ctx* h) {
    g->early.reset();
    g->early_state = HMSG_EARLY_DISCARDED;
    h->early_last = HMSG_EARLY_DISCARDED;
}
void early_unregister(hmsg_graph* g, hmsg_ctx* h) {
    if (h->early_graph == g) h->early_graph = nullptr;
    g->registered = false;
}

// the early result when it is there, complete, and made from the instances the handle holds now
std::unique_ptr<EarlyObjects> early_take(hmsg_graph* g) {
    hmsg_ctx* h = g->h;
    if (!g->registered || h->early_graph != g) return nullptr;
    const double t0 = now_ms();
    hmsg_graph_early_join(h);               // (hmsg_pool_instances joined it on leaving: nothing to wait for)
    g->t_early_wait_ms += now_ms() - t0;
    if (!g->early) return nullptr;
    if (!g->early->ok || g->early->epoch != h->inst_epoch) {
        early_drop(g, h);
        return nullptr;
    }
    return std::move(g->early);
}

void graph_finish(hmsg_graph* g, int32_t n_labels, const float* label_feats, const char* const* label_names) {
    hmsg_ctx* h = g->h;
    DbgLaps laps("graph_finish", h->stream);
    std::unique_ptr<EarlyObjects> early = early_take(g);
    if (laps.on)
        fprintf(stderr, "[hmsg graph_finish] early objects %s: the stage ran %.3f ms, the caller waited %.3f ms for it\n",
                early ? "taken" : "not there", g->t_early_ms, g->t_early_wait_ms);
    join_workers(g);
    laps.lap("join workers");
    if (early) {
        // the stage ran beside the pooling: what is left is the commit of its instances, the labels, and the lists
        ObjStage& st = early->st;
        for (size_t r = 0; r < g->rooms.size(); ++r) g->rooms[r].views.insert(g->rooms[r].views.end(), st.room_views[r].begin(), st.room_views[r].end());
        for (auto& v : st.views) g->views.push_back(std::move(v));
        laps.lap("view nodes");
        if (!h->inst_denoised) {
            if (st.have_den) hmsg_denoise_commit(h, st.den);
            h->inst_denoised = true;
        }
        g->early_state = h->early_last = HMSG_EARLY_CONSUMED;
        h->nodes.clear();
        hmsg_node_labels(h, label_feats ? n_labels : 0, label_feats);
        h->nodes = std::move(st.nodes);
        for (hmsg_node& nd : h->nodes) nd.label = h->node_label[(size_t)nd.instance];
        laps.lap("label similarity");
        add_objects(g, h->nodes, (int64_t)h->nodes.size(), n_labels, label_names);
        laps.lap("object nodes (host)");
        link_views(g, st.pair_obj, st.pair_view, st.vis, st.md);
        laps.lap("view lists (host)");
    } else {
        std::vector<std::vector<int>> room_views;
        make_views(g, g->views, room_views);
        for (size_t r = 0; r < g->rooms.size(); ++r) g->rooms[r].views.insert(g->rooms[r].views.end(), room_views[r].begin(), room_views[r].end());
        laps.lap("view nodes");
        // objects
        RoomTables t;
        room_tables(g, t);
        need(hmsg_build_object_nodes(h, (int32_t)g->floors.size(), t.fz.data(), t.fh.data(), (int32_t)g->rooms.size(), t.room_floor.data(), t.voff.data(),
                                     t.verts.data(), label_feats ? n_labels : 0, label_feats),
             h, "hmsg_build_object_nodes");
        laps.lap("hmsg_build_object_nodes");
        const int64_t N = hmsg_num_nodes(h);
        std::vector<hmsg_node> nodes((size_t)std::max<int64_t>(N, 1));
        if (N) need(hmsg_get_nodes(h, nodes.data(), nullptr), h, "hmsg_get_nodes");
        add_objects(g, nodes, N, n_labels, label_names);
        laps.lap("object nodes (host)");
        // view <-> object topology (:1712-1734): every (object, view of its room) pair in object order
        std::vector<int32_t> pair_inst, pair_view;
        std::vector<int> pair_obj;
        for (size_t k = 0; k < g->objects.size(); ++k)
            for (int v : g->rooms[(size_t)g->objects[k].room].views) {
                pair_obj.push_back((int)k);
                pair_inst.push_back(g->objects[k].instance);
                pair_view.push_back(v);
            }
        if (!pair_obj.empty()) {
            const size_t NV = g->views.size();
            std::vector<double> pinv;
            std::vector<int32_t> wh;
            view_cameras(g, h, g->views, pinv, wh);
            HMSG_REQUIRE(h->have_K, HMSG_ERR_INVALID, "hmsg_graph_finish: no camera intrinsics (hmsg_add_frames)");
            std::vector<uint8_t> vis(pair_obj.size());
            std::vector<double> md(pair_obj.size());
            need(hmsg_object_views(h, (int32_t)NV, pinv.data(), wh.data(), h->K, (int64_t)pair_obj.size(), pair_inst.data(), pair_view.data(),
                                   g->prm.min_visible_ratio, g->prm.max_view_depth, vis.data(), md.data()),
                 h, "hmsg_object_views");
            laps.lap("hmsg_object_views");
            link_views(g, pair_obj, pair_view, vis, md);
        }
        laps.lap("view lists (host)");
    }
    for (auto& o : g->objects) {
        for (int v : o.views) o.view_ids.push_back(g->views[(size_t)v].id);
        if (o.best_view >= 0) o.best_view_id = g->views[(size_t)o.best_view].id, o.have_best = true;
    }
    for (auto& v : g->views)
        for (int k : v.objects) {
            v.object_ids.push_back(g->objects[(size_t)k].id);
            v.texts.push_back(g->objects[(size_t)k].name);
        }
    if (g->prm.merge_objects_graph && !g->objects.empty()) {
        std::vector<hmsg_node> nodes(g->objects.size());
        std::vector<float> node_emb(g->objects.size() * (size_t)g->D);
        need(hmsg_get_nodes(h, nodes.data(), node_emb.data()), h, "hmsg_get_nodes");
        graph_merge_objects(g, node_emb);
    }
    laps.lap("id / text lists (host)");
    // edges (create_graph_new): a freshly built View carries an int room index, so no Room - View edge (view_room = -1)
    std::vector<int32_t> obj_room, view_room(g->views.size(), -1), vobj;
    std::vector<int64_t> vooff(1, 0);
    std::vector<int32_t> room_floor;
    for (auto& rm : g->rooms) room_floor.push_back(rm.floor);
    for (auto& o : g->objects) obj_room.push_back(o.room);
    for (auto& v : g->views) {
        vobj.insert(vobj.end(), v.objects.begin(), v.objects.end());
        vooff.push_back((int64_t)vobj.size());
    }
    int64_t ne = 0;
    const int64_t cap = (int64_t)g->floors.size() + (int64_t)g->rooms.size() + (int64_t)g->objects.size() + (int64_t)g->views.size() + (int64_t)vobj.size() + 4;
    g->edges.assign((size_t)cap * 2, 0);
    if (hmsg_graph_edges((int32_t)g->floors.size(), (int32_t)g->rooms.size(), room_floor.data(), (int32_t)g->objects.size(), obj_room.data(),
                         (int32_t)g->views.size(), view_room.data(), vooff.data(), vobj.data(), (int64_t*)g->edges.data(), cap, &ne) != HMSG_OK)
        throw hmsg_error{HMSG_ERR_INVALID, "hmsg_graph_edges failed"};
    g->edges.resize((size_t)ne * 2);
    laps.lap("edges");
    build_view_lists(g);
    g->finished = true;
}

// ---------------------------------------------------------------------------------------------- a small JSON reader (load side)
struct JVal {
    enum Kind { NUL, BOOL, NUM, STR, ARR, OBJ } kind = NUL;
    double num = 0;
    bool b = false;
    std::string str;
    std::vector<JVal> arr;
    std::vector<std::pair<std::string, JVal>> obj;
    const JVal* get(const char* key) const {
        for (auto& kv : obj)
            if (kv.first == key) return &kv.second;
        return nullptr;
    }
};
struct JParser {
    const char* p;
    const char* e;
    void ws() {
        while (p < e && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) ++p;
    }
    [[noreturn]] void fail(const char* what) { throw hmsg_error{HMSG_ERR_INVALID, std::string("JSON: ") + what}; }
    std::string str() {
        std::string o;
        if (p >= e || *p != '"') fail("string expected");
        ++p;
        while (p < e && *p != '"') {
            if (*p == '\\') {
                ++p;
                if (p >= e) fail("bad escape");
                switch (*p) {
                    case 'n': o += '\n'; break;
                    case 't': o += '\t'; break;
                    case 'r': o += '\r'; break;
                    case 'b': o += '\b'; break;
                    case 'f': o += '\f'; break;
                    case 'u': {
                        if (e - p < 5) fail("bad \\u");
                        unsigned cp = (unsigned)strtoul(std::string(p + 1, p + 5).c_str(), nullptr, 16);
                        p += 4;
                        if (cp >= 0xd800 && cp < 0xdc00 && e - p >= 7 && p[1] == '\\' && p[2] == 'u') {
                            const unsigned lo = (unsigned)strtoul(std::string(p + 3, p + 7).c_str(), nullptr, 16);
                            cp = 0x10000 + ((cp - 0xd800) << 10) + (lo - 0xdc00);
                            p += 6;
                        }
                        if (cp < 0x80) o += (char)cp;
                        else if (cp < 0x800) o += (char)(0xc0 | (cp >> 6)), o += (char)(0x80 | (cp & 0x3f));
                        else if (cp < 0x10000) o += (char)(0xe0 | (cp >> 12)), o += (char)(0x80 | ((cp >> 6) & 0x3f)), o += (char)(0x80 | (cp & 0x3f));
                        else o += (char)(0xf0 | (cp >> 18)), o += (char)(0x80 | ((cp >> 12) & 0x3f)), o += (char)(0x80 | ((cp >> 6) & 0x3f)), o += (char)(0x80 | (cp & 0x3f));
                        break;
                    }
                    default: o += *p;
                }
                ++p;
            } else {
                o += *p++;
            }
        }
        if (p >= e) fail("unterminated string");
        ++p;
        return o;
    }
    JVal val() {
        ws();
        JVal v;
        if (p >= e) fail("value expected");
        if (*p == '{') {
            v.kind = JVal::OBJ;
            ++p;
            ws();
            if (p < e && *p == '}') {
                ++p;
                return v;
            }
            for (;;) {
                ws();
                std::string k = str();
                ws();
                if (p >= e || *p != ':') fail("':' expected");
                ++p;
                v.obj.emplace_back(std::move(k), val());
                ws();
                if (p < e && *p == ',') {
                    ++p;
                    continue;
                }
                if (p < e && *p == '}') {
                    ++p;
                    return v;
                }
                fail("',' or '}' expected");
            }
        }
        if (*p == '[') {
            v.kind = JVal::ARR;
            ++p;
            ws();
            if (p < e && *p == ']') {
                ++p;
                return v;
            }
            for (;;) {
                v.arr.push_back(val());
                ws();
                if (p < e && *p == ',') {
                    ++p;
                    continue;
                }
                if (p < e && *p == ']') {
                    ++p;
                    return v;
                }
                fail("',' or ']' expected");
            }
        }
        if (*p == '"') {
            v.kind = JVal::STR;
            v.str = str();
            return v;
        }
        if (e - p >= 4 && !strncmp(p, "null", 4)) {
            p += 4;
            return v;
        }
        if (e - p >= 4 && !strncmp(p, "true", 4)) {
            p += 4;
            v.kind = JVal::BOOL;
            v.b = true;
            return v;
        }
        if (e - p >= 5 && !strncmp(p, "false", 5)) {
            p += 5;
            v.kind = JVal::BOOL;
            return v;
        }
        if (e - p >= 3 && !strncmp(p, "NaN", 3)) {
            p += 3;
            v.kind = JVal::NUM;
            v.num = NAN;
            return v;
        }
        if (e - p >= 8 && !strncmp(p, "Infinity", 8)) {
            p += 8;
            v.kind = JVal::NUM;
            v.num = INFINITY;
            return v;
        }
        if (e - p >= 9 && !strncmp(p, "-Infinity", 9)) {
            p += 9;
            v.kind = JVal::NUM;
            v.num = -INFINITY;
            return v;
        }
        char* end = nullptr;
        v.num = strtod(p, &end);                          // (correctly rounded, as Python's float())
        if (end == p) fail("value expected");
        v.kind = JVal::NUM;
        p = end;
        return v;
    }
};
JVal read_json(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw hmsg_error{HMSG_ERR_INVALID, "cannot open " + path};
    std::string s;
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    fclose(f);
    JParser jp{s.data(), s.data() + s.size()};
    JVal v = jp.val();
    if (v.kind != JVal::OBJ) throw hmsg_error{HMSG_ERR_INVALID, path + ": not a JSON object"};
    return v;
}
// Open3D read_point_cloud of the files this path writes (and of Open3D's own): hmsg_stage_files.h
std::vector<double> read_ply(const std::string& path) {
    std::vector<double> out;
    std::string msg;
    long long n = 0;
    const int rc = stage_read_ply(path, true, &n, &out, &msg);
    if (rc != STAGE_OK) throw hmsg_error{rc, msg};
    return out;
}
std::vector<std::string> list_dir(const std::string& dir, const char* suffix) {     // sorted(os.listdir(dir)) [endswith(suffix)]
    std::vector<std::string> v;
    DIR* d = opendir(dir.c_str());
    if (!d) throw hmsg_error{HMSG_ERR_INVALID, "graph not found in " + dir};
    while (dirent* e = readdir(d)) {
        std::string n = e->d_name;
        if (n == "." || n == "..") continue;
        if (suffix && (n.size() < strlen(suffix) || n.compare(n.size() - strlen(suffix), strlen(suffix), suffix) != 0)) continue;
        v.push_back(n);
    }
    closedir(d);
    std::sort(v.begin(), v.end());
    return v;
}
std::string stem_of(const std::string& file) { return file.substr(0, file.find('.')); }     // f.split(".")[0]
std::string id_text(const JVal* v) {                                                       // an id as Python would str() it
    if (!v) return "";
    if (v->kind == JVal::STR) return v->str;
    if (v->kind == JVal::NUM) {
        char b[40];
        if (v->num == std::floor(v->num) && std::fabs(v->num) < 1e15) snprintf(b, sizeof b, "%lld", (long long)v->num);
        else snprintf(b, sizeof b, "%.17g", v->num);
        return b;
    }
    return "";
}
void numbers_2d(const JVal* v, std::vector<double>& out, int* rows, int* cols) {
    out.clear();
    *rows = *cols = 0;
    if (!v || v->kind != JVal::ARR) return;
    *rows = (int)v->arr.size();
    for (auto& r : v->arr) {
        if (r.kind == JVal::ARR) {
            *cols = (int)r.arr.size();
            for (auto& x : r.arr) out.push_back(x.num);
        } else {
            out.push_back(r.num);
            *cols = 1;
        }
    }
}

void mkdirs(const std::string& p) {
    for (size_t i = 1; i <= p.size(); ++i)
        if (i == p.size() || p[i] == '/') {
            const std::string sub = p.substr(0, i);
            if (mkdir(sub.c_str(), 0777) != 0 && errno != EEXIST) throw hmsg_error{HMSG_ERR_INVALID, "cannot create " + sub};
        }
}
void write_json_fields(const std::string& path, std::vector<hmsg_json_field>& f) {
    if (hmsg_write_json(path.c_str(), (int32_t)f.size(), f.data()) != HMSG_OK) throw hmsg_error{HMSG_ERR_INVALID, "cannot write " + path};
}
hmsg_json_field raw(const char* key, const std::string& text) { return hmsg_json_field{key, HMSG_JSON_RAW, 0, 0, 0, text.c_str()}; }
hmsg_json_field num0(const char* key, const double* v) { return hmsg_json_field{key, HMSG_JSON_F64, 0, 0, 0, v}; }

}  // namespace

// ---------------------------------------------------------------------------------- the object stage beside the pooling
// hmsg_pool_instances is MFMA-bound and asks little of the memory system; the per-object DBSCAN, the room shares and the view test
// are bound by L2 latency and atomics and need only the merged instances and the room level.  The stage therefore runs while the
// pooling does, on a host thread and a normal-priority stream of its own, and leaves its result in the graph; the handle is not
// written before hmsg_graph_finish commits (between the two calls every getter answers as it did before).
int hmsg_graph_early_mode() {
    const char* e = getenv("HMSG_GRAPH_EARLY_OBJECTS");        // (read at every call: the A/B switch inside one build)
    if (!e || !*e) return 1;
    return e[0] == '0' ? 0 : (e[0] == '2' ? 2 : 1);
}

void hmsg_graph_early_start(hmsg_ctx* h) {
    hmsg_graph* g = h->early_graph;
    if (!g || !g->registered || g->h != h || !g->begun || g->finished || g->failed || !h->merged || h->restored) return;
    if (hmsg_graph_early_mode() == 0) return;
    if (g->early) {
        if (g->early->th.joinable()) return;                              // (running: hmsg_pool_instances is not re-entered)
        if (g->early->ok && g->early->epoch == h->inst_epoch) return;     // a second pooling of the same instances: the result stands
        g->early.reset();
    }
    g->early.reset(new EarlyObjects());
    EarlyObjects* e = g->early.get();
    e->epoch = h->inst_epoch;
    ++g_early_threads;
    e->th = std::thread([g, h, e] {
        const double t0 = now_ms();
        hipStream_t s = nullptr;
        // the merge fold's allocator cache is idle (its worker was joined before h->merged was set) and warm: the stage's scratch comes
        // from it and goes back to it, apart from the calling thread's cache
        dev_cache().swap_state(h->fold_cache);
        try {
            if (getenv("HMSG_DEBUG_EARLY_OBJECTS_THROW")) throw hmsg_error{HMSG_ERR_INVALID, "early object stage: HMSG_DEBUG_EARLY_OBJECTS_THROW"};
            HIP_TRY(hipSetDevice(h->cfg.device_id));
            HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));     // normal priority: the Gram beside it is the critical part
            join_workers(g);                                                 // the views come from the room level
            object_stage(g, h, s, e->st);
            HIP_TRY(hipStreamSynchronize(s));
            e->ok = true;
        } catch (...) {          // not reported: hmsg_graph_finish recomputes, and an error surfaces where it does without this stage
            if (s) (void)hipStreamSynchronize(s);
            (void)hipGetLastError();
            e->st.den.pts.release();      // (into the cache it came from)
        }
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
        h->fold_cache.swap_state(dev_cache());
        e->run_ms = now_ms() - t0;
    });
}

void hmsg_graph_early_join(hmsg_ctx* h) noexcept {
    hmsg_graph* g = h->early_graph;
    if (!g || !g->early || !g->early->th.joinable()) return;
    const double t0 = now_ms();
    g->early->th.join();
    --g_early_threads;
    g->t_early_ms = g->early->run_ms;
    const bool ok = g->early->ok;
    if (getenv("HMSG_DEBUG_TIMING"))
        fprintf(stderr, "[hmsg early objects] the stage ran %.3f ms (%s); joining it took %.3f ms\n", g->early->run_ms, ok ? "complete" : "gave up",
                now_ms() - t0);
    if (ok) g->early_state = h->early_last = HMSG_EARLY_PENDING;
    else early_drop(g, h);          // (hmsg_graph_finish recomputes; an error surfaces there, where it does without this stage)
}

void hmsg_graph_early_abort(hmsg_ctx* h) noexcept {
    hmsg_graph* g = h->early_graph;
    if (!g) return;
    hmsg_graph_early_join(h);
    if (!g->finished) early_drop(g, h);
    early_unregister(g, h);
}

extern "C" int hmsg_test_graph_early_objects(const hmsg_graph_t* g, const hmsg_t* h, int32_t* state, int32_t* live_threads) {
    if (!g && !h) return HMSG_ERR_INVALID;
    if (state) *state = g ? g->early_state : h->early_last;
    if (live_threads) *live_threads = g_early_threads.load();
    return HMSG_OK;
}

// ================================================================================================= C ABI
extern "C" {

void hmsg_graph_default_params(hmsg_graph_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->num_views = 24;              /* graph.py:1136 */
    p->kmeans_n_init = 5;           /* graph_utils.py:329-333 */
    p->kmeans_max_iter = 100;
    p->kmeans_seed = 0;
    p->skip_frames = 1;
    p->image_width = p->image_height = 0;
    p->min_visible_ratio = 0.5;     /* graph_utils.py:95-157 defaults */
    p->max_view_depth = 10.0;
    p->host_threads = 0;
    p->merge_objects_graph = 0;     /* false in every shipped config */
    p->kmeans_device = 0;           /* the fits on host threads */
}

const char* hmsg_graph_last_error(const hmsg_graph_t* g) { return g ? g->err.c_str() : "null graph"; }

void hmsg_graph_destroy(hmsg_graph_t* g) { delete g; }

int hmsg_graph_begin(hmsg_t* h, const hmsg_graph_params* prm, int32_t n_frames, const double* poses, const double* poses_inv, const float* view_feats,
                     const char* const* img_paths, hmsg_graph_t** out) {
    if (!h || !out) return HMSG_ERR_INVALID;
    *out = nullptr;
    if (n_frames < 0 || (n_frames > 0 && (!poses || !view_feats))) {
        h->err = "hmsg_graph_begin: poses / view features missing";
        return HMSG_ERR_INVALID;
    }
    hmsg_graph* g = nullptr;
    const int rc = hmsg_boundary(&h->err, -1, [&] {
        g = new hmsg_graph();
        const double t0 = now_ms();
        HMSG_REQUIRE(h->map_ready, HMSG_ERR_INVALID, "hmsg_graph_begin: finalize the map first");
        g->h = h;
        g->device = h->cfg.device_id;
        g->D = h->cfg.feat_dim;
        if (prm) g->prm = *prm;
        else hmsg_graph_default_params(&g->prm);
        if (g->prm.skip_frames <= 0) g->prm.skip_frames = h->cfg.skip_frames > 0 ? h->cfg.skip_frames : 1;
        HMSG_REQUIRE(g->prm.num_views >= 1, HMSG_ERR_INVALID, "hmsg_graph_begin: num_views");
        g->n_frames = n_frames;
        g->poses.assign(poses, poses + (size_t)n_frames * 16);
        if (poses_inv) {
            g->poses_inv.assign(poses_inv, poses_inv + (size_t)n_frames * 16);
            g->have_inv = true;
        }
        g->feats.assign(view_feats, view_feats + (size_t)n_frames * g->D);
        if (img_paths)
            for (int i = 0; i < n_frames; ++i) g->img_paths.push_back(img_paths[i] ? img_paths[i] : "");
        // floors (A8)
        int32_t nf = 0;
        need(hmsg_segment_floors(h, nullptr, 0, &nf), h, "hmsg_segment_floors");
        std::vector<hmsg_floor> fl((size_t)std::max(nf, 1));
        if (nf) need(hmsg_segment_floors(h, fl.data(), nf, &nf), h, "hmsg_segment_floors");
        for (int i = 0; i < nf; ++i) {
            GFloor f;
            f.id = std::to_string(i);
            f.name = "floor_" + std::to_string(i);
            f.f = fl[(size_t)i];
            floor_vertices(f);
            g->floors.push_back(std::move(f));
        }
        // the room level's device stage, storey by storey
        for (int i = 0; i < nf; ++i) room_level_prepare(g, i);
        // its second stage on worker threads: the rooms are independent fits
        if (g->prm.kmeans_device) {
            // one worker, so that begin returns before the fits are done; what its allocator cache holds goes back to the driver when
            // it ends (the cache belongs to the thread)
            g->workers.emplace_back([g] {
                try {
                    for (const GFloor& fl : g->floors) storey_embed_device(g, fl);
                } catch (...) {
                    hmsg_error e = hmsg_current_error();
                    std::lock_guard<std::mutex> lk(g->worker_mu);
                    if (g->worker_err.empty()) g->worker_err.swap(e.msg);
                }
                dev_cache().trim();
            });
            g->begun = true;
            g->t_begin_ms = now_ms() - t0;
            return;
        }
        std::vector<int> todo;
        for (size_t r = 0; r < g->rooms.size(); ++r) todo.push_back((int)r);
        int nt = g->prm.host_threads > 0 ? g->prm.host_threads : (int)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
        nt = std::max(1, std::min<int>(nt, (int)todo.size()));
        for (int t = 0; t < nt && !todo.empty(); ++t)
            g->workers.emplace_back([g, t, nt, todo] {
                try {
                    for (size_t k = (size_t)t; k < todo.size(); k += (size_t)nt) room_embed(g, g->rooms[(size_t)todo[k]]);
                } catch (...) {      // (kept for hmsg_graph_finish, which joins the workers and reports it)
                    hmsg_error e = hmsg_current_error();
                    std::lock_guard<std::mutex> lk(g->worker_mu);
                    if (g->worker_err.empty()) g->worker_err.swap(e.msg);
                }
            });
        g->begun = true;
        g->t_begin_ms = now_ms() - t0;
    });
    if (rc != HMSG_OK) {
        delete g;
        return rc;
    }
    // the scene knows its graph in flight, so that hmsg_pool_instances can start the object stage beside itself; a graph begun on
    // the scene before loses its place (and whatever its stage had made): it finishes by its own run of the stage
    hmsg_graph_early_abort(h);
    h->early_graph = g;
    g->registered = true;
    h->early_last = HMSG_EARLY_NEVER_MADE;
    *out = g;
    return HMSG_OK;
}

int hmsg_graph_finish(hmsg_graph_t* g, int32_t n_labels, const float* label_feats, const char* const* label_names) {
    if (!g) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g->err, -1, [&] {
        HMSG_REQUIRE(!g->failed, HMSG_ERR_INVALID, "hmsg_graph_finish: an earlier hmsg_graph_finish failed half way; destroy the graph and begin again");
        HMSG_REQUIRE(g->begun && !g->finished && g->h, HMSG_ERR_INVALID, "hmsg_graph_finish: hmsg_graph_begin first (once)");
        // everything that can be checked is checked before the graph is touched: a call that fails here can be repeated
        HMSG_REQUIRE(g->h->pooled, HMSG_ERR_INVALID, "hmsg_graph_finish: run hmsg_pool_instances first");
        HMSG_REQUIRE(g->h->have_K, HMSG_ERR_INVALID, "hmsg_graph_finish: no camera intrinsics (hmsg_add_frames)");
        const double t0 = now_ms();
        try {
            graph_finish(g, n_labels, label_feats, label_names);
        } catch (...) {
            g->failed = true;
            g->early.reset();
            early_unregister(g, g->h);
            throw;
        }
        early_unregister(g, g->h);
        g->t_finish_ms = now_ms() - t0;
    });
}

int hmsg_build_graph(hmsg_t* h, const hmsg_graph_params* prm, int32_t n_frames, const double* poses, const double* poses_inv, const float* view_feats,
                     const char* const* img_paths, int32_t n_labels, const float* label_feats, const char* const* label_names, hmsg_graph_t** out) {
    int rc = hmsg_graph_begin(h, prm, n_frames, poses, poses_inv, view_feats, img_paths, out);
    if (rc != HMSG_OK) return rc;
    rc = hmsg_graph_finish(*out, n_labels, label_feats, label_names);
    if (rc != HMSG_OK) {
        h->err = (*out)->err;
        delete *out;
        *out = nullptr;
    }
    return rc;
}

int hmsg_graph_get_counts(const hmsg_graph_t* g, hmsg_graph_counts* c) {
    if (!g || !c) return HMSG_ERR_INVALID;
    c->floors = (int32_t)g->floors.size();
    c->rooms = (int32_t)g->rooms.size();
    c->views = (int32_t)g->views.size();
    c->objects = (int32_t)g->objects.size();
    c->edges = (int64_t)(g->edges.size() / 2);
    int64_t vo = 0;
    for (auto& v : g->views) vo += (int64_t)(g->loaded ? v.object_ids.size() : v.objects.size());
    c->view_object_links = vo;
    c->begin_ms = g->t_begin_ms;
    c->finish_ms = g->t_finish_ms;
    c->kmeans_wait_ms = g->t_kmeans_wait_ms;
    return HMSG_OK;
}

int hmsg_graph_get_edges(const hmsg_graph_t* g, int64_t* edges, int64_t capacity, int64_t* n_edges) {
    if (!g || !n_edges) return HMSG_ERR_INVALID;
    *n_edges = (int64_t)(g->edges.size() / 2);
    if (!edges) return HMSG_OK;
    if (capacity < *n_edges) return HMSG_ERR_INVALID;
    memcpy(edges, g->edges.data(), g->edges.size() * 8);
    return HMSG_OK;
}

int hmsg_graph_get_objects(const hmsg_graph_t* g, hmsg_graph_object* out, int64_t capacity) {
    if (!g || !out || capacity < (int64_t)g->objects.size()) return HMSG_ERR_INVALID;
    for (size_t k = 0; k < g->objects.size(); ++k) {
        const GObject& o = g->objects[k];
        hmsg_graph_object& r = out[k];
        memset(&r, 0, sizeof r);
        snprintf(r.object_id, sizeof r.object_id, "%s", o.id.c_str());
        snprintf(r.name, sizeof r.name, "%s", o.name.c_str());
        r.room = o.room;
        r.instance = o.instance;
        r.label = o.label;
        r.n_views = (int32_t)(g->loaded ? o.view_ids.size() : o.views.size());
        r.best_view = o.best_view;
    }
    return HMSG_OK;
}

int hmsg_graph_get_rooms(const hmsg_graph_t* g, hmsg_graph_room* out, int64_t capacity) {
    if (!g || !out || capacity < (int64_t)g->rooms.size()) return HMSG_ERR_INVALID;
    for (size_t k = 0; k < g->rooms.size(); ++k) {
        const GRoom& rm = g->rooms[k];
        hmsg_graph_room& r = out[k];
        memset(&r, 0, sizeof r);
        snprintf(r.room_id, sizeof r.room_id, "%s", rm.id.c_str());
        snprintf(r.name, sizeof r.name, "%s", rm.name.c_str());
        r.floor = rm.floor;
        r.n_vertices = (int64_t)(rm.verts.size() / 2);
        r.n_points = (int64_t)(g->loaded ? rm.pts.size() / 3 : rm.sel.size());
        r.n_embeddings = rm.n_emb;
        r.n_sample_images = (int32_t)rm.sample.size();
        r.n_objects = (int32_t)rm.objects.size();
        r.n_views = (int32_t)(g->loaded ? rm.view_ids.size() : rm.views.size());
    }
    return HMSG_OK;
}

int hmsg_graph_get_room_vertices(const hmsg_graph_t* g, int32_t room, double* xz, int64_t capacity) {
    if (!g || room < 0 || room >= (int32_t)g->rooms.size() || !xz) return HMSG_ERR_INVALID;
    const GRoom& rm = g->rooms[(size_t)room];
    if ((size_t)capacity < rm.verts.size()) return HMSG_ERR_INVALID;
    if (!rm.verts.empty()) memcpy(xz, rm.verts.data(), rm.verts.size() * 8);
    return HMSG_OK;
}

int hmsg_graph_get_room_embeddings(const hmsg_graph_t* g, int32_t room, float* emb, int64_t capacity) {
    if (!g || room < 0 || room >= (int32_t)g->rooms.size() || !emb) return HMSG_ERR_INVALID;
    const GRoom& rm = g->rooms[(size_t)room];
    const size_t n = (size_t)rm.n_emb * (size_t)g->D;
    if ((size_t)capacity < n) return HMSG_ERR_INVALID;
    if (g->loaded)
        for (size_t i = 0; i < n; ++i) emb[i] = (float)rm.emb64[i];
    else if (n) memcpy(emb, rm.emb.data(), n * 4);
    return HMSG_OK;
}

/* the whole topology as one JSON text (ids, names, lists): what a test or a scripting host compares / walks */
int hmsg_graph_to_json(const hmsg_graph_t* g, char* buf, int64_t capacity, int64_t* needed) {
    if (!g || !needed) return HMSG_ERR_INVALID;
    return hmsg_boundary(nullptr, -1, [&] {
        std::string s = "{\"floors\": [";
        for (size_t i = 0; i < g->floors.size(); ++i) {
            const GFloor& f = g->floors[i];
            if (i) s += ", ";
            std::vector<std::string> rids;
            for (int r : f.rooms) rids.push_back(g->rooms[(size_t)r].id);
            s += "{\"floor_id\": " + jstr(f.id) + ", \"name\": " + jstr(f.name) + ", \"rooms\": " + jlist(rids) + ", \"n_points\": " +
                 std::to_string((long long)(g->loaded ? (long long)(f.pts.size() / 3) : (long long)f.f.n_points)) + "}";
        }
        s += "], \"rooms\": [";
        for (size_t i = 0; i < g->rooms.size(); ++i) {
            const GRoom& r = g->rooms[i];
            if (i) s += ", ";
            std::vector<std::string> oids, vids;
            for (int o : r.objects) oids.push_back(g->objects[(size_t)o].id);
            if (g->loaded) vids = r.view_ids;
            else
                for (int v : r.views) vids.push_back(g->views[(size_t)v].id);
            s += "{\"room_id\": " + jstr(r.id) + ", \"name\": " + jstr(r.name) + ", \"floor_id\": " + jstr(g->floors[(size_t)r.floor].id) + ", \"objects\": " +
                 jlist(oids) + ", \"views\": " + jlist(vids) + ", \"represent_images\": [";
            for (size_t k = 0; k < r.represent.size(); ++k) s += (k ? ", " : "") + std::to_string(r.represent[k]);
            s += "], \"sample_images\": [";
            for (size_t k = 0; k < r.sample.size(); ++k) s += (k ? ", " : "") + std::to_string(r.sample[k]);
            s += "], \"n_points\": " + std::to_string((long long)(g->loaded ? r.pts.size() / 3 : r.sel.size())) + ", \"n_vertices\": " +
                 std::to_string((long long)(r.verts.size() / 2)) + ", \"n_embeddings\": " + std::to_string(r.n_emb) + "}";
        }
        s += "], \"views\": [";
        for (size_t i = 0; i < g->views.size(); ++i) {
            const GView& v = g->views[i];
            if (i) s += ", ";
            s += "{\"view_id\": " + jstr(v.id) + ", \"room_id\": " + (g->loaded ? jstr(v.room_id_str) : std::to_string(v.room_in_floor)) + ", \"img_id\": " +
                 (v.have_img ? std::to_string(v.img) : std::string("null")) + ", \"object_ids\": " + jlist(v.object_ids) + ", \"img_path\": " +
                 (v.have_path ? jstr(v.img_path) : std::string("null")) + ", \"text_discription\": " + jlist(v.texts) + "}";
        }
        s += "], \"objects\": [";
        for (size_t i = 0; i < g->objects.size(); ++i) {
            const GObject& o = g->objects[i];
            if (i) s += ", ";
            s += "{\"object_id\": " + jstr(o.id) + ", \"room_id\": " + jstr(o.room_id) + ", \"name\": " + jstr(o.name) + ", \"instance\": " +
                 std::to_string(o.instance) + ", \"label\": " + std::to_string(o.label) + ", \"view_ids\": " + jlist(o.view_ids) + ", \"best_view_id\": " +
                 (o.have_best ? jstr(o.best_view_id) : std::string("null")) + "}";
        }
        s += "], \"edges\": [";
        for (size_t i = 0; i + 1 < g->edges.size(); i += 2) s += (i ? ", [" : "[") + std::to_string(g->edges[i]) + ", " + std::to_string(g->edges[i + 1]) + "]";
        s += "]}";
        *needed = (int64_t)s.size() + 1;
        if (!buf) return;
        HMSG_REQUIRE(capacity >= *needed, HMSG_ERR_INVALID, "hmsg_graph_to_json: buf too small (see *needed)");
        memcpy(buf, s.c_str(), s.size() + 1);
    });
}

/* the navigation maps of a storey (hmsg_navmap.hip): the slab hmsg_save writes, selected on the device from the map in HBM */
static GFloor& nav_floor(hmsg_graph_t* g, int32_t floor, const char* fn) {
    const std::string f = fn;
    HMSG_REQUIRE(!g->loaded, HMSG_ERR_INVALID,
                 f + ": a graph read by hmsg_load has no cloud in HBM (give the points of hmsg_read_ply to hmsg_nav_floor_maps)");
    HMSG_REQUIRE(g->finished && g->h, HMSG_ERR_INVALID, f + ": a graph built by hmsg_build_graph / hmsg_graph_finish (its map lives in the scene handle)");
    HMSG_REQUIRE(g->h->map_ready, HMSG_ERR_INVALID, f + ": map not finalised");
    HMSG_REQUIRE(floor >= 0 && (size_t)floor < g->floors.size(), HMSG_ERR_INVALID, f + ": no such floor");
    HIP_TRY(hipSetDevice(g->h->cfg.device_id));
    HIP_TRY(hipStreamSynchronize(g->h->stream));
    return g->floors[(size_t)floor];
}
int hmsg_graph_nav_grid(hmsg_graph_t* g, int32_t floor, double cell_size, double* pcd_min, double* pcd_max, int32_t* grid) {
    if (!g || !grid) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g->err, -1, [&] {
        const GFloor& fl = nav_floor(g, floor, "hmsg_graph_nav_grid");
        hmsg_nav_grid_device("hmsg_graph_nav_grid", cell_size, (const double*)g->h->pts.p, (long long)g->h->V, fl.f.y_lo, fl.f.y_hi, pcd_min, pcd_max,
                             grid);
    });
}
int hmsg_graph_nav_floor_maps(hmsg_graph_t* g, int32_t floor, const hmsg_nav_params* prm, int32_t n_poses, const double* poses,
                              hmsg_nav_maps* out) {
    if (!g || !prm || !out) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g->err, -1, [&] {
        const GFloor& fl = nav_floor(g, floor, "hmsg_graph_nav_floor_maps");
        hmsg_nav_maps_device("hmsg_graph_nav_floor_maps", *prm, (const double*)g->h->pts.p, (const double*)g->h->cols.p, (long long)g->h->V, fl.f.y_lo,
                             fl.f.y_hi, fl.f.zero_level, n_poses, poses, out);
    });
}
int hmsg_graph_nav_height_map(hmsg_graph_t* g, int32_t floor, const hmsg_height_params* prm, uint16_t* top, uint8_t* known, double* pcd_min,
                              double* pcd_max, int32_t* grid) {
    if (!g || !prm || !top) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g->err, -1, [&] {
        const GFloor& fl = nav_floor(g, floor, "hmsg_graph_nav_height_map");
        hmsg_nav_height_device("hmsg_graph_nav_height_map", *prm, (const double*)g->h->pts.p, (long long)g->h->V, fl.f.y_lo, fl.f.y_hi,
                               fl.f.zero_level, top, known, pcd_min, pcd_max, grid);
    });
}

/* save_hmsg_graph (graph.py:1801-1824) in the reference layout: <dir>/floors, rooms, objects, views */
int hmsg_save(hmsg_graph_t* g, const char* dir) {
    if (!g || !dir) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g->err, -1, [&] {
        HMSG_REQUIRE(g->finished && g->h, HMSG_ERR_INVALID, "hmsg_save: a graph built by hmsg_build_graph / hmsg_graph_finish (its clouds live in the scene handle)");
        hmsg_ctx* h = g->h;
        const std::string root = dir;
        for (const char* sub : {"floors", "rooms", "objects", "views"}) mkdirs(root + "/" + sub);
        // the map: floors are slabs of it, room clouds selections of a slab
        const int64_t V = hmsg_map_size(h);
        std::vector<double> map((size_t)std::max<int64_t>(V, 1) * 3);
        if (V) need(hmsg_get_map_points(h, map.data(), nullptr), h, "hmsg_get_map_points");
        for (size_t fi = 0; fi < g->floors.size(); ++fi) {
            GFloor& fl = g->floors[fi];
            std::vector<double> slab;
            for (int64_t i = 0; i < V; ++i) {
                const double y = map[(size_t)i * 3 + 1];
                if (y >= fl.f.y_lo && y <= fl.f.y_hi) slab.insert(slab.end(), &map[(size_t)i * 3], &map[(size_t)i * 3 + 3]);
            }
            if (hmsg_write_ply((root + "/floors/" + fl.id + ".ply").c_str(), slab.data(), (int64_t)(slab.size() / 3)) != HMSG_OK)
                throw hmsg_error{HMSG_ERR_INVALID, "cannot write the floor cloud"};
            std::vector<std::string> rids;
            for (int r : fl.rooms) rids.push_back(g->rooms[(size_t)r].id);
            const std::string s_id = jstr(fl.id), s_name = jstr(fl.name), s_rooms = jlist(rids);
            double zeros[24] = {0};
            std::vector<hmsg_json_field> f = {raw("floor_id", s_id), raw("name", s_name), raw("rooms", s_rooms),
                                              hmsg_json_field{"vertices", HMSG_JSON_F64, 2, 8, 3, fl.have_verts ? &fl.verts[0][0] : zeros},
                                              num0("floor_height", &fl.f.height), num0("floor_zero_level", &fl.f.zero_level)};
            write_json_fields(root + "/floors/" + fl.id + ".json", f);
            for (int ri : fl.rooms) {
                GRoom& rm = g->rooms[(size_t)ri];
                std::vector<double> pts;
                pts.reserve(rm.sel.size() * 3);
                for (int s : rm.sel) pts.insert(pts.end(), &slab[(size_t)s * 3], &slab[(size_t)s * 3 + 3]);
                if (hmsg_write_ply((root + "/rooms/" + rm.id + ".ply").c_str(), pts.data(), (int64_t)(pts.size() / 3)) != HMSG_OK)
                    throw hmsg_error{HMSG_ERR_INVALID, "cannot write a room cloud"};
                std::vector<std::string> oids, vids;
                for (int o : rm.objects) oids.push_back(g->objects[(size_t)o].id);
                for (int v : rm.views) vids.push_back(g->views[(size_t)v].id);
                const std::string r_id = jstr(rm.id), r_name = jstr(rm.name), r_fl = jstr(fl.id), r_obj = jlist(oids), r_views = jlist(vids), empty = "[]";
                std::vector<hmsg_json_field> rf = {
                    raw("room_id", r_id), raw("name", r_name), raw("floor_id", r_fl), raw("objects", r_obj), raw("views", r_views),
                    hmsg_json_field{"vertices", HMSG_JSON_F64, 2, (int64_t)(rm.verts.size() / 2), 2, rm.verts.data()},
                    num0("room_height", &rm.height), num0("room_zero_level", &rm.zero),
                    rm.n_emb ? hmsg_json_field{"embeddings", HMSG_JSON_F32, 2, rm.n_emb, g->D, rm.emb.data()} : raw("embeddings", empty),
                    hmsg_json_field{"represent_images", HMSG_JSON_I64, 1, (int64_t)rm.represent.size(), 0, rm.represent.data()},
                    hmsg_json_field{"sample_images", HMSG_JSON_I64, 1, (int64_t)rm.sample.size(), 0, rm.sample.data()},
                    rm.n_clip ? hmsg_json_field{"clip_embeddings", HMSG_JSON_F32, 2, rm.n_clip, g->D, rm.clip.data()} : raw("clip_embeddings", empty)};
                if (rm.verts.empty()) rf[5] = raw("vertices", empty);
                write_json_fields(root + "/rooms/" + rm.id + ".json", rf);
            }
        }
        for (auto& v : g->views) {
            const std::string v_id = jstr(v.id), v_room = std::to_string(v.room_in_floor), v_img = std::to_string(v.img), v_obj = jlist(v.object_ids),
                              v_path = v.have_path ? jstr(v.img_path) : std::string("null"), v_txt = jlist(v.texts);
            std::vector<hmsg_json_field> vf = {raw("view_id", v_id),    raw("room_id", v_room), raw("img_id", v_img),
                                               raw("object_ids", v_obj), raw("img_path", v_path), raw("text_discription", v_txt)};
            write_json_fields(root + "/views/" + v.id + ".json", vf);
        }
        // objects: the bulk writer (clouds and features read back from HBM once, host threads print)
        std::vector<std::string> keep;
        keep.reserve(g->objects.size() * 6);
        std::vector<hmsg_object_record> recs;
        recs.reserve(g->objects.size());
        std::vector<double> inst_pts;              // (merged objects: their clouds are pieced together on the host)
        for (size_t k = 0; k < g->objects.size(); ++k) {
            const GObject& o = g->objects[k];
            if (o.parts.size() > 1) {
                // an object Room.merge_objects added others to: Object.save (object.py:37-57) of the concatenated cloud, the 8 corners of
                // its box (get_box_points' order) and the mean embedding -- what the Python mirror writes for it
                if (inst_pts.empty()) {
                    inst_pts.resize((size_t)std::max<long long>(h->inst.total, 1) * 3);
                    need(hmsg_get_instance_points(h, inst_pts.data()), h, "hmsg_get_instance_points");
                }
                std::vector<double> pts;
                for (int inst : o.parts)
                    pts.insert(pts.end(), inst_pts.begin() + (ptrdiff_t)(h->inst.off[(size_t)inst] * 3), inst_pts.begin() + (ptrdiff_t)(h->inst.off[(size_t)inst + 1] * 3));
                if (hmsg_write_ply((root + "/objects/" + o.id + ".ply").c_str(), pts.data(), (int64_t)(pts.size() / 3)) != HMSG_OK)
                    throw hmsg_error{HMSG_ERR_INVALID, "cannot write an object cloud"};
                double mn[3] = {pts[0], pts[1], pts[2]}, mx[3] = {pts[0], pts[1], pts[2]};
                for (size_t i = 0; i < pts.size(); i += 3)
                    for (int a = 0; a < 3; ++a) {
                        mn[a] = std::min(mn[a], pts[i + a]);
                        mx[a] = std::max(mx[a], pts[i + a]);
                    }
                const double ex[3] = {mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]};
                const double box[8][3] = {{mn[0], mn[1], mn[2]},         {mn[0] + ex[0], mn[1], mn[2]},         {mn[0], mn[1] + ex[1], mn[2]},
                                          {mn[0], mn[1], mn[2] + ex[2]}, {mx[0], mx[1], mx[2]},                 {mn[0], mn[1] + ex[1], mn[2] + ex[2]},
                                          {mn[0] + ex[0], mn[1], mn[2] + ex[2]}, {mn[0] + ex[0], mn[1] + ex[1], mn[2]}};
                const std::string o_id = jstr(o.id), o_room = jstr(o.room_id), o_name = jstr(o.name), o_views = jlist(o.view_ids),
                                  o_best = o.have_best ? jstr(o.best_view_id) : std::string("null");
                std::vector<hmsg_json_field> of = {raw("object_id", o_id), hmsg_json_field{"vertices", HMSG_JSON_F64, 2, 8, 3, &box[0][0]},
                                                   raw("room_id", o_room), raw("name", o_name),
                                                   hmsg_json_field{"embedding", HMSG_JSON_F32, 1, (int64_t)o.emb32.size(), 0, o.emb32.data()},
                                                   raw("view_ids", o_views), raw("best_view_id", o_best)};
                write_json_fields(root + "/objects/" + o.id + ".json", of);
                continue;
            }
            const size_t b = keep.size();
            keep.push_back(o.id);
            keep.push_back(jstr(o.id));
            keep.push_back(jstr(o.room_id));
            keep.push_back(jstr(o.name));
            keep.push_back(jlist(o.view_ids));
            keep.push_back(o.have_best ? jstr(o.best_view_id) : std::string("null"));
            recs.push_back(hmsg_object_record{o.instance, keep[b].c_str(), keep[b + 1].c_str(), keep[b + 2].c_str(), keep[b + 3].c_str(), keep[b + 4].c_str(),
                                              keep[b + 5].c_str()});
        }
        if (!recs.empty()) need(hmsg_save_objects(h, (root + "/objects").c_str(), (int64_t)recs.size(), recs.data(), g->prm.host_threads), h, "hmsg_save_objects");
    });
}

/* the reader of hmsg_load, for a host that resumes from full_pcd.ply and objects/pcd_<i>.ply (hmsg_restore_stage) */
int hmsg_read_ply(const char* path, double* xyz, int64_t capacity, int64_t* n) {
    if (!path || !n || capacity < 0) return HMSG_ERR_INVALID;
    *n = 0;
    return hmsg_boundary("hmsg_read_ply", -1, [&] {
        std::vector<double> pts;
        std::string msg;
        long long cnt = 0;
        const int rc = stage_read_ply(path, xyz != nullptr, &cnt, &pts, &msg);
        if (rc != STAGE_OK) throw hmsg_error{rc, msg};
        *n = (int64_t)cnt;
        if (!xyz) return;
        HMSG_REQUIRE(cnt <= capacity, HMSG_ERR_INVALID, std::string(path) + ": more vertices than the capacity handed in");
        if (cnt) memcpy(xyz, pts.data(), (size_t)cnt * 24);
    });
}

/* load_hmsg_graph (graph.py:1892-1987): floors, rooms, objects, views from the reference layout */
int hmsg_load(const char* dir, int32_t device_id, hmsg_graph_t** out) {
    if (!dir || !out) return HMSG_ERR_INVALID;
    *out = nullptr;
    hmsg_graph* g = nullptr;
    const int rc = hmsg_boundary("hmsg_load", -1, [&] {
        g = new hmsg_graph();
        const std::string root = dir;
        g->loaded = g->finished = true;
        g->device = device_id;
        hmsg_graph_default_params(&g->prm);
        std::map<std::string, int> room_of_id;
        for (auto& f : list_dir(root + "/floors", ".ply")) {                                  // sorted (:1903)
            GFloor fl;
            fl.id = stem_of(f);
            fl.pts = read_ply(root + "/floors/" + f);
            const JVal m = read_json(root + "/floors/" + fl.id + ".json");
            fl.name = "floor_" + fl.id;
            if (const JVal* v = m.get("name"))
                if (v->kind == JVal::STR) fl.name = v->str;                                    // (Floor.load takes the saved name)
            if (const JVal* v = m.get("floor_height")) fl.f.height = v->num;
            if (const JVal* v = m.get("floor_zero_level")) fl.f.zero_level = v->num;
            std::vector<double> vv;
            int r = 0, c = 0;
            numbers_2d(m.get("vertices"), vv, &r, &c);
            if (r == 8 && c == 3) memcpy(fl.verts, vv.data(), sizeof fl.verts), fl.have_verts = true;
            fl.f.n_points = (int64_t)(fl.pts.size() / 3);
            g->floors.push_back(std::move(fl));
        }
        for (auto& f : list_dir(root + "/rooms", ".ply")) {                                   // lexicographic (:1931)
            GRoom rm;
            rm.id = stem_of(f);
            const std::string fid = rm.id.substr(0, rm.id.find('_'));
            rm.pts = read_ply(root + "/rooms/" + f);
            const JVal m = read_json(root + "/rooms/" + rm.id + ".json");
            if (const JVal* v = m.get("name"))
                if (v->kind == JVal::STR) rm.name = v->str;
            const int fl = atoi(fid.c_str());                                                // self.floors[int(rid.split("_")[0])]
            HMSG_REQUIRE(fl >= 0 && fl < (int)g->floors.size(), HMSG_ERR_INVALID, "hmsg_load: a room of a floor that is not there");
            rm.floor = fl;
            rm.index_in_floor = (int)g->floors[(size_t)fl].rooms.size();
            int r = 0, c = 0;
            numbers_2d(m.get("vertices"), rm.verts, &r, &c);
            if (const JVal* v = m.get("room_height")) rm.height = v->num, rm.have_level = v->kind == JVal::NUM;
            if (const JVal* v = m.get("room_zero_level")) rm.zero = v->num;
            numbers_2d(m.get("embeddings"), rm.emb64, &rm.n_emb, &c);
            if (rm.n_emb) {
                HMSG_REQUIRE(g->D == 0 || g->D == c, HMSG_ERR_INVALID, "hmsg_load: embeddings of different lengths");
                g->D = c;
            }
            std::vector<double> tmp;
            numbers_2d(m.get("represent_images"), tmp, &r, &c);
            for (double x : tmp) rm.represent.push_back((long long)x);
            numbers_2d(m.get("sample_images"), tmp, &r, &c);
            for (double x : tmp) rm.sample.push_back((long long)x);
            std::vector<double> clip64;
            numbers_2d(m.get("clip_embeddings"), clip64, &rm.n_clip, &c);
            rm.clip.assign(clip64.begin(), clip64.end());
            if (const JVal* v = m.get("views"))
                for (auto& x : v->arr) rm.view_ids.push_back(id_text(&x));
            room_of_id[rm.id] = (int)g->rooms.size();
            g->floors[(size_t)fl].rooms.push_back((int)g->rooms.size());
            g->rooms.push_back(std::move(rm));
        }
        for (auto& f : list_dir(root + "/objects", ".ply")) {
            GObject o;
            o.id = stem_of(f);
            const size_t u1 = o.id.find('_'), u2 = u1 == std::string::npos ? u1 : o.id.find('_', u1 + 1);
            o.room_id = u2 == std::string::npos ? o.id : o.id.substr(0, u2);                  // "_".join(oid.split("_")[:2])
            auto it = room_of_id.find(o.room_id);
            HMSG_REQUIRE(it != room_of_id.end(), HMSG_ERR_INVALID, "hmsg_load: Couldn't find the room with room id " + o.room_id);
            o.room = it->second;
            o.pts = read_ply(root + "/objects/" + f);
            const JVal m = read_json(root + "/objects/" + o.id + ".json");
            o.name = "object_" + o.id;
            if (const JVal* v = m.get("name"))
                if (v->kind == JVal::STR) o.name = v->str;
            int r = 0, c = 0;
            numbers_2d(m.get("vertices"), o.verts, &r, &c);
            if (const JVal* v = m.get("embedding"))
                if (v->kind == JVal::ARR)
                    for (auto& x : v->arr) o.emb.push_back(x.num);
            if (!o.emb.empty()) {
                HMSG_REQUIRE(g->D == 0 || g->D == (int)o.emb.size(), HMSG_ERR_INVALID, "hmsg_load: embeddings of different lengths");
                g->D = (int)o.emb.size();
            }
            if (const JVal* v = m.get("view_ids"))
                for (auto& x : v->arr) o.view_ids.push_back(id_text(&x));
            if (const JVal* v = m.get("best_view_id"))
                if (v->kind != JVal::NUL) o.best_view_id = id_text(v), o.have_best = true;
            g->rooms[(size_t)o.room].objects.push_back((int)g->objects.size());
            g->objects.push_back(std::move(o));
        }
        std::map<std::string, int> obj_of_id;
        for (size_t k = 0; k < g->objects.size(); ++k) obj_of_id.emplace(g->objects[k].id, (int)k);     // (first of equal ids)
        for (auto& f : list_dir(root + "/views", nullptr)) {
            GView v;
            v.id = stem_of(f);
            const size_t u1 = v.id.find('_'), u2 = u1 == std::string::npos ? u1 : v.id.find('_', u1 + 1);
            v.room_id_str = u2 == std::string::npos ? v.id : v.id.substr(0, u2);
            auto it = room_of_id.find(v.room_id_str);
            HMSG_REQUIRE(it != room_of_id.end(), HMSG_ERR_INVALID, "hmsg_load: Couldn't find the room with room id " + v.room_id_str);
            const JVal m = read_json(root + "/views/" + f);
            v.floor = g->rooms[(size_t)it->second].floor;
            v.room_in_floor = g->rooms[(size_t)it->second].index_in_floor;
            if (const JVal* x = m.get("img_id")) {
                v.have_img = x->kind == JVal::NUM;
                v.img = (long long)x->num;
            }
            if (const JVal* x = m.get("img_path"))
                if (x->kind == JVal::STR) v.img_path = x->str, v.have_path = true;
            if (const JVal* x = m.get("object_ids"))
                for (auto& y : x->arr) v.object_ids.push_back(id_text(&y));
            if (const JVal* x = m.get("text_discription"))
                for (auto& y : x->arr) v.texts.push_back(id_text(&y));
            for (auto& oid : v.object_ids) {
                auto o = obj_of_id.find(oid);
                if (o != obj_of_id.end()) v.objects.push_back(o->second);
            }
            std::sort(v.objects.begin(), v.objects.end());
            v.objects.erase(std::unique(v.objects.begin(), v.objects.end()), v.objects.end());
            g->rooms[(size_t)it->second].views.push_back((int)g->views.size());
            g->views.push_back(std::move(v));
        }
        // best_view_id / view_ids -> view indices (graph.py:2759-2765 walks self.views for the id: the first view that carries it; an
        // id that names no view leaves best_view = None there, -1 here)
        std::map<std::string, int> view_of_id;
        for (size_t v = 0; v < g->views.size(); ++v) view_of_id.emplace(g->views[v].id, (int)v);
        for (auto& o : g->objects) {
            for (auto& vid : o.view_ids) {
                auto it = view_of_id.find(vid);
                if (it != view_of_id.end()) o.views.push_back(it->second);
            }
            if (o.have_best) {
                auto it = view_of_id.find(o.best_view_id);
                if (it != view_of_id.end()) o.best_view = it->second;
            }
        }
        build_view_lists(g);
        // edges as load_hmsg_graph adds them: (0, floor) per floor, (floor, room) per room, (room, object) per object, (room, view)
        // per view -- the loader adds no View - Object edge
        const long long F = (long long)g->floors.size(), R = (long long)g->rooms.size(), O = (long long)g->objects.size();
        for (long long i = 0; i < F; ++i) g->edges.push_back(0), g->edges.push_back(1 + i);
        for (long long r = 0; r < R; ++r) g->edges.push_back(1 + g->rooms[(size_t)r].floor), g->edges.push_back(1 + F + r);
        for (long long o = 0; o < O; ++o) g->edges.push_back(1 + F + g->objects[(size_t)o].room), g->edges.push_back(1 + F + R + o);
        for (size_t v = 0; v < g->views.size(); ++v) {
            const int r = room_of_id[g->views[v].room_id_str];
            g->edges.push_back(1 + F + r);
            g->edges.push_back(1 + F + R + O + (long long)v);
        }
    });
    if (rc != HMSG_OK) {
        delete g;
        return rc;
    }
    *out = g;
    return HMSG_OK;
}

}  // extern "C"

// ---- hmsg_graph_evaluate: evaluate_floors / _rooms / _objects (hm3dsem_evaluator.py:193-589) of a built or a loaded graph
namespace {

struct EvalScene {                          // a loaded graph has no scene handle: a small one for the call's device work
    hmsg_t* h = nullptr;
    ~EvalScene() {
        if (h) hmsg_destroy(h);
    }
};

void graph_evaluate(hmsg_graph* g, const hmsg_eval_gt* gt, const hmsg_eval_params* prm_in, hmsg_eval_metrics* out, double* top_k_acc) {
    HMSG_REQUIRE(gt && out, HMSG_ERR_INVALID, "hmsg_graph_evaluate: null argument");
    HMSG_REQUIRE(g->finished && !g->failed, HMSG_ERR_INVALID, "hmsg_graph_evaluate: the graph is not finished");
    hmsg_eval_params prm;
    hmsg_eval_default_params(&prm);
    if (prm_in) prm = *prm_in;
    HMSG_REQUIRE(prm.eval_metric == HMSG_EVAL_IOU || prm.eval_metric == HMSG_EVAL_OVERLAP, HMSG_ERR_INVALID, "hmsg_graph_evaluate: unknown eval_metric");
    HMSG_REQUIRE(prm.n_top_k >= 0 && (prm.n_top_k == 0 || (prm.top_k && top_k_acc)), HMSG_ERR_INVALID, "hmsg_graph_evaluate: a top_k list without top_k_acc");
    hmsg_eval_metrics m;
    memset(&m, 0, sizeof m);
    hmsg_ctx* h = g->h;
    EvalScene own;
    if (!h) {
        hmsg_config cfg;
        hmsg_default_config(&cfg);
        cfg.device_id = g->device;
        cfg.feat_dim = 16, cfg.height = cfg.width = 8, cfg.max_frames = 1, cfg.max_masks = 1;
        if (hmsg_create(&cfg, &own.h) != HMSG_OK) throw hmsg_error{HMSG_ERR_INVALID, "hmsg_graph_evaluate: cannot make a scene handle on the graph's device"};
        h = own.h;
    }
    const bool built = g->h != nullptr && !g->loaded;
    // ---- floors
    {
        const size_t Fp = g->floors.size();
        std::vector<double> verts(std::max<size_t>(Fp, 1) * 24, 0.0);
        for (size_t f = 0; f < Fp; ++f) {
            HMSG_REQUIRE(g->floors[f].have_verts, HMSG_ERR_INVALID, "hmsg_graph_evaluate: floor " + g->floors[f].id + " has no vertices");
            memcpy(&verts[f * 24], g->floors[f].verts, sizeof(double) * 24);
        }
        HMSG_REQUIRE(gt->n_floors == (int32_t)Fp && Fp > 0, HMSG_ERR_INVALID,
                     "hmsg_graph_evaluate: " + std::to_string(gt->n_floors) + " ground-truth floors against " + std::to_string(Fp) +
                         " predicted (the reference raises there)");
        if (hmsg_eval_floors(gt->floor_lower, gt->floor_upper, gt->n_floors, verts.data(), (int32_t)Fp, &m.floors) != HMSG_OK)
            throw hmsg_error{HMSG_ERR_INVALID, "hmsg_graph_evaluate: hmsg_eval_floors refused its arguments"};
    }
    // ---- rooms: the clouds as hmsg_save fetches them (built: selections of a storey's slab of the map; loaded: as read)
    {
        const int32_t P = (int32_t)g->rooms.size(), G = gt->n_rooms;
        HMSG_REQUIRE(P > 0 && G > 0, HMSG_ERR_INVALID, "hmsg_graph_evaluate: no predicted or no ground-truth rooms");
        std::vector<std::vector<double>> cloud((size_t)P);
        if (built) {
            const int64_t V = hmsg_map_size(h);
            std::vector<double> map((size_t)std::max<int64_t>(V, 1) * 3);
            if (V) need(hmsg_get_map_points(h, map.data(), nullptr), h, "hmsg_get_map_points");
            for (const GFloor& fl : g->floors) {
                std::vector<double> slab;
                for (int64_t i = 0; i < V; ++i) {
                    const double y = map[(size_t)i * 3 + 1];
                    if (y >= fl.f.y_lo && y <= fl.f.y_hi) slab.insert(slab.end(), &map[(size_t)i * 3], &map[(size_t)i * 3 + 3]);
                }
                for (int ri : fl.rooms) {
                    const GRoom& rm = g->rooms[(size_t)ri];
                    cloud[(size_t)ri].reserve(rm.sel.size() * 3);
                    for (int s : rm.sel) cloud[(size_t)ri].insert(cloud[(size_t)ri].end(), &slab[(size_t)s * 3], &slab[(size_t)s * 3 + 3]);
                }
            }
        }
        std::vector<double> pts, zl((size_t)P), ht((size_t)P);
        std::vector<int64_t> off((size_t)P + 1, 0);
        for (int32_t p = 0; p < P; ++p) {
            const GRoom& rm = g->rooms[(size_t)p];
            const std::vector<double>& c = built ? cloud[(size_t)p] : rm.pts;
            pts.insert(pts.end(), c.begin(), c.end());
            off[(size_t)p + 1] = (int64_t)(pts.size() / 3);
            zl[(size_t)p] = rm.zero, ht[(size_t)p] = rm.height;
        }
        const size_t PG = (size_t)P * (size_t)G;
        std::vector<double> assoc(PG), over_pred(PG), over_gt(PG);
        need(hmsg_eval_rooms(h, P, pts.data(), off.data(), zl.data(), ht.data(), G, gt->room_pts, gt->room_off, gt->room_min_h, gt->room_max_h,
                             gt->room_mean_h, gt->n_floors, gt->floor_lower, gt->floor_upper, prm.voxel, prm.room_radius, assoc.data(),
                             over_pred.data(), over_gt.data(), nullptr),
             h, "hmsg_eval_rooms");
        std::vector<int32_t> row((size_t)std::min(P, G)), col((size_t)std::min(P, G));
        int32_t n = 0;
        need(hmsg_eval_hydra_means(over_pred.data(), over_gt.data(), P, G, &m.room_hydra_prec, &m.room_hydra_recall), nullptr, "hmsg_eval_hydra_means");
        need(hmsg_lsap(P, G, assoc.data(), 1, row.data(), col.data(), &n), nullptr, "hmsg_lsap");
        need(hmsg_eval_metrics_from_matrix(assoc.data(), P, G, row.data(), col.data(), n, 6, &m.room_ap, &m.room_acc50, &m.room_prec50, &m.room_recall50),
             nullptr, "hmsg_eval_metrics_from_matrix");
        m.room_gt = G, m.room_pred = P;
    }
    // ---- objects
    {
        const int32_t P = (int32_t)g->objects.size(), G = gt->n_objects, C = gt->n_classes, D = g->D;
        HMSG_REQUIRE(P > 0 && G > 0, HMSG_ERR_INVALID, "hmsg_graph_evaluate: no predicted or no ground-truth objects");
        HMSG_REQUIRE(C > 0 && gt->feat_dim == D && gt->text_feats && gt->class_name_id && gt->obj_name_id, HMSG_ERR_INVALID,
                     "hmsg_graph_evaluate: the class table is missing or its feat_dim (" + std::to_string(gt->feat_dim) + ") is not the graph's (" +
                         std::to_string(D) + ")");
        std::vector<double> pts, emb64;
        std::vector<float> emb32;
        std::vector<int64_t> off((size_t)P + 1, 0);
        if (built) {
            const int64_t N = hmsg_num_instances(h);
            std::vector<double> ip((size_t)std::max<long long>(h->inst.total, 1) * 3);
            std::vector<float> feats((size_t)std::max<int64_t>(N, 1) * (size_t)D);
            need(hmsg_get_instance_points(h, ip.data()), h, "hmsg_get_instance_points");
            need(hmsg_get_instance_feats(h, feats.data()), h, "hmsg_get_instance_feats");
            emb32.resize((size_t)P * (size_t)D);
            for (int32_t p = 0; p < P; ++p) {
                const GObject& o = g->objects[(size_t)p];
                const std::vector<int> one = {o.instance};
                for (int inst : (o.parts.empty() ? one : o.parts)) {
                    HMSG_REQUIRE(inst >= 0 && inst < N, HMSG_ERR_INVALID, "hmsg_graph_evaluate: object " + o.id + " names an instance the scene no longer has");
                    pts.insert(pts.end(), ip.begin() + (ptrdiff_t)(h->inst.off[(size_t)inst] * 3), ip.begin() + (ptrdiff_t)(h->inst.off[(size_t)inst + 1] * 3));
                }
                off[(size_t)p + 1] = (int64_t)(pts.size() / 3);
                if (o.parts.size() > 1 || !o.emb32.empty()) {
                    HMSG_REQUIRE((int32_t)o.emb32.size() == D, HMSG_ERR_INVALID, "hmsg_graph_evaluate: object " + o.id + " has no embedding");
                    memcpy(&emb32[(size_t)p * D], o.emb32.data(), (size_t)D * 4);
                } else {
                    memcpy(&emb32[(size_t)p * D], &feats[(size_t)o.instance * D], (size_t)D * 4);
                }
            }
        } else {
            emb64.resize((size_t)P * (size_t)D);
            for (int32_t p = 0; p < P; ++p) {
                const GObject& o = g->objects[(size_t)p];
                pts.insert(pts.end(), o.pts.begin(), o.pts.end());
                off[(size_t)p + 1] = (int64_t)(pts.size() / 3);
                HMSG_REQUIRE((int32_t)o.emb.size() == D, HMSG_ERR_INVALID, "hmsg_graph_evaluate: object " + o.id + " has no embedding");
                memcpy(&emb64[(size_t)p * D], o.emb.data(), (size_t)D * 8);
            }
        }
        const size_t PG = (size_t)P * (size_t)G;
        std::vector<double> iou(PG), ov(PG);
        need(hmsg_eval_object_matrices(h, P, pts.data(), off.data(), G, gt->obj_pts, gt->obj_off, gt->obj_obb_center, gt->obj_obb_dims, prm.object_radius,
                                       iou.data(), ov.data(), nullptr),
             h, "hmsg_eval_object_matrices");
        std::vector<int32_t> row((size_t)std::min(P, G)), col((size_t)std::min(P, G));
        int32_t n = 0;
        need(hmsg_lsap(P, G, prm.eval_metric == HMSG_EVAL_IOU ? iou.data() : ov.data(), 1, row.data(), col.data(), &n), nullptr, "hmsg_lsap");
        // the sweep and the recount at 0.5 read the OVERLAP matrix under either assignment (:473, :499)
        need(hmsg_eval_metrics_from_matrix(ov.data(), P, G, row.data(), col.data(), n, 6, &m.obj_ap, nullptr, nullptr, nullptr), nullptr,
             "hmsg_eval_metrics_from_matrix");
        need(hmsg_eval_counts_at(ov.data(), P, G, row.data(), col.data(), n, 0.5, &m.obj_iou50), nullptr, "hmsg_eval_counts_at");
        m.obj_gt = G, m.obj_pred = P, m.obj_assigned = n;
        // top-k semantics of EVERY assigned pair (:567)
        std::vector<int32_t> target((size_t)n), rank((size_t)n);
        const size_t rb = built ? 4 : 8;
        std::vector<unsigned char> sel((size_t)n * (size_t)D * rb);
        const unsigned char* src = built ? (const unsigned char*)emb32.data() : (const unsigned char*)emb64.data();
        for (int32_t k = 0; k < n; ++k) {
            target[(size_t)k] = gt->obj_name_id[col[(size_t)k]];
            memcpy(&sel[(size_t)k * D * rb], src + (size_t)row[(size_t)k] * D * rb, (size_t)D * rb);
        }
        need(hmsg_eval_semantic_ranks(h, n, sel.data(), built ? 0 : 1, D, C, gt->text_feats, gt->class_name_id, target.data(), rank.data()), h,
             "hmsg_eval_semantic_ranks");
        need(hmsg_eval_top_k(rank.data(), n, C, prm.top_k, prm.n_top_k, top_k_acc, &m.obj_top_k_auc), nullptr, "hmsg_eval_top_k");
    }
    *out = m;
}

}  // namespace

extern "C" {

void hmsg_eval_default_params(hmsg_eval_params* p) {
    if (!p) return;
    p->eval_metric = HMSG_EVAL_OVERLAP;
    p->room_radius = 0.05;
    p->object_radius = 0.02;
    p->voxel = 0.05;
    p->n_top_k = 0;
    p->top_k = nullptr;
}

int hmsg_graph_evaluate(hmsg_graph_t* g, const hmsg_eval_gt* gt, const hmsg_eval_params* prm, hmsg_eval_metrics* out, double* top_k_acc) {
    if (!g) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g->err, -1, [&] { graph_evaluate(g, gt, prm, out, top_k_acc); });
}

}  // extern "C"

namespace {
// hmsg_graph_index; rooms_only: the levels above the nodes into an index without a node table (a graph without objects)
void graph_make_index(hmsg_graph* g, const double* room_name_emb, bool rooms_only, hmsg_index_t** out) {
    HMSG_REQUIRE(g->finished, HMSG_ERR_INVALID, "hmsg_graph_index: the graph is not finished");
    HMSG_REQUIRE(rooms_only || !g->objects.empty(), HMSG_ERR_INVALID, "hmsg_graph_index: a graph without objects");
    hmsg_index_t* ix = nullptr;
    const int D = g->D;
    if (rooms_only) {
        ix = hmsg_index_create_rooms_only(g->device, D);
    } else if (!g->loaded && !g->merged) {
        need(hmsg_index_from_nodes(g->h, &ix), g->h, "hmsg_index_from_nodes");
    } else if (g->merged && !g->loaded) {
        // merged objects are no rows of the scene's node table any more: the table of the graph's own objects
        std::vector<float> emb(g->objects.size() * (size_t)D);
        std::vector<int32_t> room(g->objects.size());
        for (size_t k = 0; k < g->objects.size(); ++k) {
            memcpy(&emb[k * (size_t)D], g->objects[k].emb32.data(), (size_t)D * 4);
            room[k] = g->objects[k].room;
        }
        if (hmsg_index_create(g->device, D, (int64_t)g->objects.size(), emb.data(), 0, room.data(), &ix) != HMSG_OK)
            throw hmsg_error{HMSG_ERR_INVALID, "hmsg_index_create failed"};
    } else {
        std::vector<double> emb(g->objects.size() * (size_t)D);
        std::vector<int32_t> room(g->objects.size());
        for (size_t k = 0; k < g->objects.size(); ++k) {
            HMSG_REQUIRE((int)g->objects[k].emb.size() == D, HMSG_ERR_INVALID, "hmsg_graph_index: object " + g->objects[k].id + " was saved without an embedding");
            memcpy(&emb[k * (size_t)D], g->objects[k].emb.data(), (size_t)D * 8);
            room[k] = g->objects[k].room;
        }
        if (hmsg_index_create(g->device, D, (int64_t)g->objects.size(), emb.data(), 1, room.data(), &ix) != HMSG_OK)
            throw hmsg_error{HMSG_ERR_INVALID, "hmsg_index_create failed"};
    }
    const int R = (int)g->rooms.size();
    std::vector<int32_t> fro(1, 0), fr, key((size_t)R);
    for (auto& fl : g->floors) {
        for (int r : fl.rooms) fr.push_back(r);
        fro.push_back((int32_t)fr.size());
    }
    std::vector<int64_t> voff(1, 0);
    std::vector<double> vemb;
    for (int r = 0; r < R; ++r) {
        const GRoom& rm = g->rooms[(size_t)r];
        const size_t us = rm.id.rfind('_');
        key[(size_t)r] = atoi(rm.id.c_str() + (us == std::string::npos ? 0 : us + 1));
        if (g->loaded) vemb.insert(vemb.end(), rm.emb64.begin(), rm.emb64.end());
        else
            for (float x : rm.emb) vemb.push_back((double)x);
        voff.push_back(voff.back() + rm.n_emb);
    }
    const int rc = hmsg_index_set_hierarchy(ix, R, (int32_t)g->floors.size(), fro.data(), fr.data(), room_name_emb, voff.data(), vemb.empty() ? nullptr : vemb.data(),
                                            key.data());
    if (rc != HMSG_OK) {
        std::string e = hmsg_index_last_error(ix);
        hmsg_index_destroy(ix);
        throw hmsg_error{rc, "hmsg_index_set_hierarchy: " + e};
    }
    *out = ix;
}
}  // namespace

extern "C" {

/* the retrieval index of the graph with its upper levels resident (Graph._hier_index of the mirror): object embeddings (gathered
 * on the device for a built graph, the saved float64 rows for a loaded one), floors -> rooms, the rooms' view embeddings,
 * room_key = int(room_id.split("_")[-1]); room_name_emb f64 [rooms][D] or NULL (no label mode) */
int hmsg_graph_index(hmsg_graph_t* g, const double* room_name_emb, hmsg_index_t** out) {
    if (!g || !out) return HMSG_ERR_INVALID;
    *out = nullptr;
    return hmsg_boundary(&g->err, -1, [&] { graph_make_index(g, room_name_emb, false, out); });
}

}  // extern "C"

// (hmsg_query_sharded.hip) the graph as one shard of the sharded query: its own resident index, made on first use WITHOUT room
// names (the sharded calls pass them every time) -- for a graph without objects one with the levels above the nodes only; the
// index of hmsg_graph_query stays as that call makes it.  Throws what makes the graph no shard (not finished, failed half way, no
// embedding length).  *n_floor_rooms: the length of the floors' room lists.
hmsg_index_t* hmsg_graph_shard_index(hmsg_graph* g, int* n_floor_rooms) {
    *n_floor_rooms = 0;
    for (auto& fl : g->floors) *n_floor_rooms += (int)fl.rooms.size();
    HMSG_REQUIRE(g->finished && !g->failed, HMSG_ERR_INVALID, "hmsg_graph_query_sharded: a graph built by hmsg_graph_finish or loaded by hmsg_load");
    HMSG_REQUIRE(g->D > 0, HMSG_ERR_INVALID, "hmsg_graph_query_sharded: the graph has no embeddings (D unknown)");
    if (!g->shard_ix) graph_make_index(g, nullptr, g->objects.empty(), &g->shard_ix);
    return g->shard_ix;
}
hmsg_shard_ws*& hmsg_graph_shard_ws(hmsg_graph* g) { return g->shard_ws; }
int hmsg_graph_device(const hmsg_graph* g) { return g->device; }
void hmsg_graph_set_error(hmsg_graph* g, const std::string& e) { g->err = e; }
// (hmsg_comm.hip)
struct hmsg_comm;
void hmsg_comm_allgather_bytes(hmsg_ctx* h, hmsg_comm* c, const void* mine, size_t my_bytes, std::vector<std::vector<char>>& all);
int hmsg_comm_rank(const hmsg_comm* c);
int hmsg_comm_world(const hmsg_comm* c);
void hmsg_comm_set_error(hmsg_comm* c, const std::string& e);
extern "C" {

/* configs[3], cross-scene retrieval with the levels above the nodes: every rank's graph -> ONE resident index on every rank.  The node
 * tables travel as in hmsg_allgather_nodes (embeddings gathered on the device, HBM to HBM); the hierarchy -- floors -> rooms, the
 * rooms' keys, their view embeddings and (optionally, on every rank or on none) the embeddings of their names -- as one small table per
 * rank.  Global ids: node = node_off[rank] + local, room = room_off[rank] + local, floor = floor_off[rank] + local ([world + 1] each,
 * optional); a query names its storey by the global floor id.  Until round 5 the benchmark gathered these tables as pickled Python
 * objects (torch.distributed.all_gather_object) inside its timed step. */
int hmsg_graph_allgather_index(hmsg_graph_t* g, hmsg_comm_t* c, const double* room_name_emb, hmsg_index_t** out, int64_t* node_off, int64_t* room_off,
                               int64_t* floor_off) {
    if (!g || !c || !out) return HMSG_ERR_INVALID;
    *out = nullptr;
    const int rc = hmsg_boundary(&g->err, -1, [&] {
        HMSG_REQUIRE(g->finished && g->h && !g->loaded, HMSG_ERR_INVALID, "hmsg_graph_allgather_index: a graph built by hmsg_graph_finish");
        HMSG_REQUIRE(!g->merged, HMSG_ERR_UNSUPPORTED, "hmsg_graph_allgather_index: not with merge_objects_graph (the merged objects are no rows of the scene's node table)");
        hmsg_ctx* h = g->h;
        const int D = g->D, W = hmsg_comm_world(c), me = hmsg_comm_rank(c);
        const int R = (int)g->rooms.size(), F = (int)g->floors.size();
        // this rank's table: header | floor_room_off | floor_rooms | room_key | view_off | names | views
        std::vector<int64_t> hdr = {F, R, 0, room_name_emb ? 1 : 0}, fro(1, 0), fr, key((size_t)R), voff(1, 0);
        std::vector<double> vemb;
        for (auto& fl : g->floors) {
            for (int r : fl.rooms) fr.push_back(r);
            fro.push_back((int64_t)fr.size());
        }
        for (int r = 0; r < R; ++r) {
            const GRoom& rm = g->rooms[(size_t)r];
            const size_t us = rm.id.rfind('_');
            key[(size_t)r] = atoi(rm.id.c_str() + (us == std::string::npos ? 0 : us + 1));
            for (float x : rm.emb) vemb.push_back((double)x);
            voff.push_back(voff.back() + rm.n_emb);
        }
        hdr[2] = voff.back();
        std::vector<char> blob;
        auto put = [&](const void* p, size_t n) { blob.insert(blob.end(), (const char*)p, (const char*)p + n); };
        put(hdr.data(), 32);
        put(fro.data(), fro.size() * 8);
        put(fr.data(), fr.size() * 8);
        put(key.data(), key.size() * 8);
        put(voff.data(), voff.size() * 8);
        if (room_name_emb) put(room_name_emb, (size_t)R * D * 8);
        put(vemb.data(), vemb.size() * 8);
        // the node tables first (its own agreement step makes every rank fail together on a bad table)
        std::vector<int64_t> noff((size_t)W + 1, 0), roff((size_t)W + 1, 0);
        hmsg_index_t* ix = nullptr;
        const int rn = hmsg_allgather_nodes(h, c, R, &ix, noff.data(), roff.data());
        if (rn != HMSG_OK) throw hmsg_error{rn, h->err};
        std::vector<std::vector<char>> all;
        try {
            hmsg_comm_allgather_bytes(h, c, blob.data(), blob.size(), all);
            std::vector<int32_t> g_fro(1, 0), g_fr, g_key;
            std::vector<int64_t> g_voff(1, 0), foff((size_t)W + 1, 0);
            std::vector<double> g_names, g_views;
            bool names_all = true, names_any = false;
            for (int r = 0; r < W; ++r) {
                const char* p = all[(size_t)r].data();
                HMSG_REQUIRE(all[(size_t)r].size() >= 32, HMSG_ERR_INVALID, "hmsg_graph_allgather_index: a rank sent no table");
                const int64_t* hd = (const int64_t*)p;
                const int64_t Fr = hd[0], Rr = hd[1], NVr = hd[2], hn = hd[3];
                HMSG_REQUIRE(Rr == roff[(size_t)r + 1] - roff[(size_t)r], HMSG_ERR_INVALID, "hmsg_graph_allgather_index: room counts of the two exchanges differ");
                const int64_t* q = hd + 4;
                const int64_t* r_fro = q;
                q += Fr + 1;
                const int64_t* r_fr = q;
                q += r_fro[Fr];
                const int64_t* r_key = q;
                q += Rr;
                const int64_t* r_voff = q;
                q += Rr + 1;
                const double* r_names = (const double*)q;
                const double* r_views = r_names + (hn ? (size_t)Rr * D : 0);
                names_all = names_all && hn != 0;
                names_any = names_any || hn != 0;
                for (int64_t f = 0; f < Fr; ++f) {
                    for (int64_t k = r_fro[f]; k < r_fro[f + 1]; ++k) g_fr.push_back((int32_t)(r_fr[k] + roff[(size_t)r]));
                    g_fro.push_back((int32_t)g_fr.size());
                }
                foff[(size_t)r + 1] = foff[(size_t)r] + Fr;
                for (int64_t k = 0; k < Rr; ++k) {
                    g_key.push_back((int32_t)r_key[k]);
                    g_voff.push_back(g_voff.back() + (r_voff[k + 1] - r_voff[k]));
                }
                if (hn) g_names.insert(g_names.end(), r_names, r_names + (size_t)Rr * D);
                g_views.insert(g_views.end(), r_views, r_views + (size_t)NVr * D);
            }
            HMSG_REQUIRE(names_all || !names_any, HMSG_ERR_INVALID, "hmsg_graph_allgather_index: room name embeddings on every rank or on none");
            const int rs = hmsg_index_set_hierarchy(ix, (int32_t)roff[(size_t)W], (int32_t)foff[(size_t)W], g_fro.data(), g_fr.data(), names_all ? g_names.data() : nullptr,
                                                    g_voff.data(), g_views.empty() ? nullptr : g_views.data(), g_key.data());
            if (rs != HMSG_OK) throw hmsg_error{rs, std::string("hmsg_index_set_hierarchy: ") + hmsg_index_last_error(ix)};
            for (int r = 0; r <= W; ++r) {
                if (node_off) node_off[r] = noff[(size_t)r];
                if (room_off) room_off[r] = roff[(size_t)r];
                if (floor_off) floor_off[r] = foff[(size_t)r];
            }
            (void)me;
        } catch (...) {
            hmsg_index_destroy(ix);
            throw;
        }
        *out = ix;
    });
    if (rc != HMSG_OK) hmsg_comm_set_error(c, g->err);
    return rc;
}

/* query_hierarchy_protected{,_icra} (graph.py:3483-3716) on the graph: hmsg_query_hier on its index (made on the first call, with
 * room_name_emb; pass the same table on later calls or NULL) */
int hmsg_graph_query(hmsg_graph_t* g, const double* room_name_emb, int32_t Q, int32_t C, const float* T_obj, const int32_t* qid, const float* T_room,
                     const int32_t* floor_id, const int32_t* room_mode, int32_t k, int32_t use_negatives, int32_t max_rooms, int32_t* out_sel,
                     int32_t* out_nsel, int32_t* out_idx, int32_t* out_room, double* out_score) {
    if (!g) return HMSG_ERR_INVALID;
    if (!g->ix) {
        const int rc = hmsg_graph_index(g, room_name_emb, &g->ix);
        if (rc != HMSG_OK) return rc;
    }
    const int rc = hmsg_query_hier(g->ix, Q, C, T_obj, qid, T_room, floor_id, room_mode, k, use_negatives, max_rooms, out_sel, out_nsel, out_idx, out_room,
                                   out_score);
    if (rc != HMSG_OK) g->err = hmsg_index_last_error(g->ix);
    return rc;
}

/* Graph.generate_room_names (graph.py:2146-2187) on the graph object: "obj_embedding" (Room.infer_room_type_from_objects, room.py:237-308)
 * or "view_embedding" (Room.infer_room_type_from_view_embedding, room.py:131-172) -- hmsg_roomnames.hip.  All rooms are named in one
 * batch, and only once every room has an answer (a room without objects fails the whole call, as the reference's loop raises there). */
int hmsg_graph_name_rooms(hmsg_graph_t* g, int32_t method, int32_t n_types, const float* type_feats, const char* const* type_names,
                          int32_t* type_of_room) {
    if (!g) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g->err, -1, [&] {
        HMSG_REQUIRE(g->finished && !g->failed, HMSG_ERR_INVALID, "hmsg_graph_name_rooms: the graph is not finished");
        HMSG_REQUIRE(method == HMSG_ROOM_NAMES_OBJ_EMBEDDING || method == HMSG_ROOM_NAMES_VIEW_EMBEDDING, HMSG_ERR_INVALID,
                     "hmsg_graph_name_rooms: unknown method (\"label\" asks an LLM: not on the device)");
        HMSG_REQUIRE(n_types >= 1 && type_feats && type_names, HMSG_ERR_INVALID, "hmsg_graph_name_rooms: no room types");
        for (int t = 0; t < n_types; ++t) HMSG_REQUIRE(type_names[t] != nullptr, HMSG_ERR_INVALID, "hmsg_graph_name_rooms: a type without a name");
        const int R = (int)g->rooms.size(), D = g->D;
        std::vector<int32_t> type((size_t)std::max(R, 1), -1);
        if (R > 0) {
            HMSG_REQUIRE(D > 0, HMSG_ERR_INVALID, "hmsg_graph_name_rooms: the graph has no embeddings");
            HIP_TRY(hipSetDevice(g->h ? g->h->cfg.device_id : g->device));
            if (g->h) HIP_TRY(hipStreamSynchronize(g->h->stream));
            hipStream_t s = nullptr;
            DevBuf<float> d_T;
            d_T.alloc((size_t)n_types * D);
            HIP_TRY(hipMemcpyAsync(d_T.p, type_feats, (size_t)n_types * D * 4, hipMemcpyHostToDevice, s));
            if (method == HMSG_ROOM_NAMES_OBJ_EMBEDDING) {
                std::vector<long long> off(1, 0);
                for (const GRoom& rm : g->rooms) {
                    HMSG_REQUIRE(!rm.objects.empty(), HMSG_ERR_INVALID,
                                 "hmsg_graph_name_rooms: room " + rm.id + " has no objects (feats_denoise_dbscan of an empty array raises); no room was renamed");
                    off.push_back(off.back() + (long long)rm.objects.size());
                }
                const long long N = off.back();
                const bool f64 = g->loaded;
                DevBuf<char> X, rep;
                X.alloc((size_t)N * D * (f64 ? 8 : 4));
                rep.alloc((size_t)R * D * (f64 ? 8 : 4));
                if (f64) {                                            // json.load's float64 rows (object.py:88)
                    std::vector<double> h((size_t)N * D);
                    size_t at = 0;
                    for (const GRoom& rm : g->rooms)
                        for (int o : rm.objects) {
                            const GObject& ob = g->objects[(size_t)o];
                            HMSG_REQUIRE((int)ob.emb.size() == D, HMSG_ERR_INVALID, "hmsg_graph_name_rooms: object " + ob.id + " was saved without an embedding");
                            memcpy(&h[at], ob.emb.data(), (size_t)D * 8);
                            at += (size_t)D;
                        }
                    HIP_TRY(hipMemcpyAsync(X.p, h.data(), h.size() * 8, hipMemcpyHostToDevice, s));
                } else if (g->merged) {                               // Room.merge_objects' mean embeddings (host float32)
                    std::vector<float> h((size_t)N * D);
                    size_t at = 0;
                    for (const GRoom& rm : g->rooms)
                        for (int o : rm.objects) {
                            memcpy(&h[at], g->objects[(size_t)o].emb32.data(), (size_t)D * 4);
                            at += (size_t)D;
                        }
                    HIP_TRY(hipMemcpyAsync(X.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, s));
                } else {                                              // the pooled features, gathered in HBM
                    std::vector<int> rows;
                    rows.reserve((size_t)N);
                    for (const GRoom& rm : g->rooms)
                        for (int o : rm.objects) rows.push_back(g->objects[(size_t)o].instance);
                    rn_gather_rows_f32(s, g->h->inst_feats.p, rows, D, (float*)X.p);
                }
                rn_denoise(s, X.p, f64, D, off, 0.02, 2, rep.p, nullptr);
                DevBuf<int> d_type;
                d_type.alloc((size_t)R);
                rn_choose(s, rep.p, f64, R, D, d_T.p, n_types, d_type.p);
                HIP_TRY(hipMemcpyAsync(type.data(), d_type.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
            } else {
                std::vector<long long> voff(1, 0);
                for (const GRoom& rm : g->rooms) voff.push_back(voff.back() + rm.n_emb);
                const long long NV = voff.back();
                if (NV > 0) {
                    const bool f64 = g->loaded;
                    DevBuf<char> V;
                    V.alloc((size_t)NV * D * (f64 ? 8 : 4));
                    size_t at = 0;
                    for (const GRoom& rm : g->rooms) {
                        const size_t n = (size_t)rm.n_emb * D;
                        if (!n) continue;
                        HIP_TRY(hipMemcpyAsync(V.p + at, f64 ? (const void*)rm.emb64.data() : (const void*)rm.emb.data(), n * (f64 ? 8 : 4),
                                               hipMemcpyHostToDevice, s));
                        at += n * (f64 ? 8 : 4);
                    }
                    DevBuf<int> d_vt;
                    d_vt.alloc((size_t)NV);
                    rn_choose(s, V.p, f64, NV, D, d_T.p, n_types, d_vt.p);
                    rn_vote(s, d_vt.p, voff, n_types, type.data());
                }
            }
        }
        for (int r = 0; r < R; ++r)                                   // (a room without views keeps its name: room.py:153-155)
            if (type[(size_t)r] >= 0) g->rooms[(size_t)r].name = type_names[type[(size_t)r]];
        if (type_of_room)
            for (int r = 0; r < R; ++r) type_of_room[r] = type[(size_t)r];
        if (g->ix) {                                                  // label mode answers from the names: the next query re-indexes
            hmsg_index_destroy(g->ix);
            g->ix = nullptr;
        }
    });
}

/* Graph.set_room_names (graph.py:2129-2144) */
int hmsg_graph_set_room_names(hmsg_graph_t* g, int32_t n, const char* const* names) {
    if (!g) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g->err, -1, [&] {
        HMSG_REQUIRE(n == (int32_t)g->rooms.size(), HMSG_ERR_INVALID, "hmsg_graph_set_room_names: The length of room_names should be the same as the number of rooms in the graph");
        HMSG_REQUIRE(n == 0 || names, HMSG_ERR_INVALID, "hmsg_graph_set_room_names: no names");
        for (int r = 0; r < n; ++r) HMSG_REQUIRE(names[r] != nullptr, HMSG_ERR_INVALID, "hmsg_graph_set_room_names: a NULL name");
        for (int r = 0; r < n; ++r) g->rooms[(size_t)r].name = names[r];
        if (g->ix) {
            hmsg_index_destroy(g->ix);
            g->ix = nullptr;
        }
    });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- the view level of the slow path
// Graph.query_room_obj_slow_reasoning (graph.py:2578-3054) between its VLM calls; the device side is hmsg_query_views.hip.
namespace {
void views_ready(const hmsg_graph* g, const char* who) {
    HMSG_REQUIRE(g->finished && !g->failed, HMSG_ERR_INVALID, std::string(who) + ": a graph built by hmsg_graph_finish or loaded by hmsg_load");
}
int view_room(const hmsg_graph* g, const GView& v) {
    if (v.floor < 0 || v.floor >= (int)g->floors.size()) return -1;
    const auto& rooms = g->floors[(size_t)v.floor].rooms;
    return v.room_in_floor >= 0 && v.room_in_floor < (int)rooms.size() ? rooms[(size_t)v.room_in_floor] : -1;
}
hipStream_t view_stream(hmsg_graph* g) {
    HIP_TRY(hipSetDevice(g->device));
    if (!g->view_stream) HIP_TRY(hipStreamCreateWithFlags(&g->view_stream, hipStreamNonBlocking));
    return g->view_stream;
}
hmsg_goal_table* goal_table(hmsg_graph* g) {
    if (g->goal) return g->goal;
    const int R = (int)g->rooms.size();
    int D = g->D;
    std::vector<int> img_off(1, 0), fro(1, 0), fr;
    std::vector<float> clip;
    std::vector<long long> img_id;
    g->goal_bad.assign((size_t)R, "");
    for (int r = 0; r < R; ++r) {
        const GRoom& rm = g->rooms[(size_t)r];
        if (rm.n_clip > 0 && D <= 0) D = (int)(rm.clip.size() / (size_t)rm.n_clip);
        if ((size_t)rm.n_clip != rm.sample.size())
            g->goal_bad[(size_t)r] = "room " + rm.id + ": Number of images (" + std::to_string(rm.sample.size()) + ") != embeddings (" + std::to_string(rm.n_clip) + ")";
        else if (rm.n_clip > 0 && rm.clip.size() != (size_t)rm.n_clip * (size_t)D)
            g->goal_bad[(size_t)r] = "room " + rm.id + ": clip_embeddings of another length than the graph's embeddings";
        if (g->goal_bad[(size_t)r].empty()) {
            clip.insert(clip.end(), rm.clip.begin(), rm.clip.end());
            img_id.insert(img_id.end(), rm.sample.begin(), rm.sample.end());
        }
        img_off.push_back((int)img_id.size());
    }
    for (auto& fl : g->floors) {
        for (int r : fl.rooms) fr.push_back(r);
        fro.push_back((int)fr.size());
    }
    g->goal = hmsg_goal_table_create(g->device, std::max(D, 1), R, img_off, clip, img_id, fro, fr);
    return g->goal;
}
// the clouds of objects obj[0 .. n) as segments of one device buffer: the instance clouds in the scene's HBM for a built graph (the
// concatenated parts after merge_objects_graph), GObject::pts uploaded once for a loaded one.  obj -1: an empty cloud.
const double* object_clouds(hmsg_graph* g, hipStream_t s, int n, const int* obj, std::vector<long long>& seg_off, std::vector<CloudSeg>& segs) {
    seg_off.assign(1, 0);
    segs.clear();
    const double* base = nullptr;
    if (g->loaded) {
        if (!g->have_obj_pts) {
            g->obj_pts_off.assign(1, 0);
            for (auto& o : g->objects) g->obj_pts_off.push_back(g->obj_pts_off.back() + (long long)(o.pts.size() / 3));
            HIP_TRY(hipSetDevice(g->device));
            g->obj_pts.alloc((size_t)std::max<long long>(g->obj_pts_off.back(), 1) * 3);
            for (size_t k = 0; k < g->objects.size(); ++k)
                if (!g->objects[k].pts.empty()) h2d_bounce(g->obj_pts.p + (size_t)g->obj_pts_off[k] * 3, g->objects[k].pts.data(), g->objects[k].pts.size() / 3 * 24, s);
            HIP_TRY(hipStreamSynchronize(s));
            g->have_obj_pts = true;
        }
        base = g->obj_pts.p;
    } else {
        HMSG_REQUIRE(g->h != nullptr, HMSG_ERR_INVALID, "the graph has no scene handle");
        base = g->h->inst.pts.p;
    }
    for (int i = 0; i < n; ++i) {
        if (obj[i] >= 0) {
            const GObject& o = g->objects[(size_t)obj[i]];
            if (g->loaded) {
                segs.push_back(CloudSeg{g->obj_pts_off[(size_t)obj[i]], g->obj_pts_off[(size_t)obj[i] + 1] - g->obj_pts_off[(size_t)obj[i]]});
            } else {
                const std::vector<int> one(1, o.instance);
                for (int part : (g->merged ? o.parts : one)) {
                    HMSG_REQUIRE(part >= 0 && (size_t)part + 1 < g->h->inst.off.size(), HMSG_ERR_INVALID, "an object without an instance cloud");
                    segs.push_back(CloudSeg{g->h->inst.off[(size_t)part], g->h->inst.off[(size_t)part + 1] - g->h->inst.off[(size_t)part]});
                }
            }
        }
        seg_off.push_back((long long)segs.size());
    }
    return base;
}
}  // namespace

extern "C" {

int hmsg_graph_get_views(hmsg_graph_t* g, hmsg_graph_view* out, int64_t capacity) {
    if (!g) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g->err, -1, [&] {
        views_ready(g, "hmsg_graph_get_views");
        HMSG_REQUIRE(capacity >= (int64_t)g->views.size() && (out || g->views.empty()), HMSG_ERR_INVALID, "hmsg_graph_get_views: capacity too small");
        const auto& lists = g->view_lists;
        for (size_t v = 0; v < g->views.size(); ++v) {
            const GView& w = g->views[v];
            hmsg_graph_view& r = out[v];
            memset(&r, 0, sizeof r);
            r.view = (int32_t)v;
            r.room = view_room(g, w);
            r.img_id = w.have_img ? (int64_t)w.img : -1;
            r.n_objects = (int32_t)lists[v].size();
        }
    });
}

int hmsg_graph_get_view_objects(hmsg_graph_t* g, int32_t view, int32_t* obj, int64_t capacity) {
    if (!g) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g->err, -1, [&] {
        views_ready(g, "hmsg_graph_get_view_objects");
        HMSG_REQUIRE(view >= 0 && view < (int32_t)g->views.size(), HMSG_ERR_INVALID, "hmsg_graph_get_view_objects: view index out of range");
        const auto& l = g->view_lists[(size_t)view];
        HMSG_REQUIRE(l.empty() || (obj && capacity >= (int64_t)l.size()), HMSG_ERR_INVALID, "hmsg_graph_get_view_objects: capacity too small");
        if (!l.empty()) memcpy(obj, l.data(), l.size() * 4);
    });
}

/* find_view_by_imgpath (graph.py:2566-2570): the first view, in view order, with that path (img_path non-NULL) or that image id */
int hmsg_graph_find_view(hmsg_graph_t* g, const char* img_path, int64_t img_id, int32_t* view) {
    if (!g || !view) return HMSG_ERR_INVALID;
    *view = -1;
    return hmsg_boundary(&g->err, -1, [&] {
        views_ready(g, "hmsg_graph_find_view");
        for (size_t v = 0; v < g->views.size(); ++v) {
            const GView& w = g->views[v];
            if (img_path ? (w.have_path && w.img_path == img_path) : (w.have_img && (int64_t)w.img == img_id)) {
                *view = (int32_t)v;
                break;
            }
        }
    });
}

/* graph.py:2759-2765 and :2828-2831: best_object.best_view_id -> the view that carries it -> its img_id */
int hmsg_graph_object_best_views(hmsg_graph_t* g, int32_t n, const int32_t* obj, int32_t* view, int64_t* img_id) {
    if (!g) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g->err, -1, [&] {
        views_ready(g, "hmsg_graph_object_best_views");
        HMSG_REQUIRE(n >= 0 && (n == 0 || (obj && view)), HMSG_ERR_INVALID, "hmsg_graph_object_best_views: bad argument");
        for (int i = 0; i < n; ++i) HMSG_REQUIRE(obj[i] >= 0 && obj[i] < (int32_t)g->objects.size(), HMSG_ERR_INVALID, "hmsg_graph_object_best_views: object index out of range");
        for (int i = 0; i < n; ++i) {
            const int bv = g->objects[(size_t)obj[i]].best_view;
            view[i] = bv;
            if (img_id) img_id[i] = bv >= 0 && g->views[(size_t)bv].have_img ? (int64_t)g->views[(size_t)bv].img : -1;
        }
    });
}

/* graph.py:2864-2897 for Q queries at once */
int hmsg_graph_goal_views(hmsg_graph_t* g, int32_t Q, const float* T, const int32_t* floor_id, int32_t k, int64_t* out_img, int32_t* out_room,
                          double* out_score, int32_t* out_n) {
    if (!g) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g->err, -1, [&] {
        views_ready(g, "hmsg_graph_goal_views");
        HMSG_REQUIRE(Q >= 0 && k >= 1 && (Q == 0 || (T && floor_id && out_img && out_room && out_score && out_n)), HMSG_ERR_INVALID,
                     "hmsg_graph_goal_views: bad argument");
        if (Q == 0) return;
        hmsg_goal_table* t = goal_table(g);
        std::vector<char> seen(g->floors.size() + 1, 0);
        for (int q = 0; q < Q; ++q) {
            const int f = floor_id[q];
            HMSG_REQUIRE(f >= -1 && f < (int)g->floors.size(), HMSG_ERR_INVALID, "hmsg_graph_goal_views: floor id out of range");
            if (seen[(size_t)(f + 1)]) continue;
            seen[(size_t)(f + 1)] = 1;
            if (f < 0) {
                for (auto& why : g->goal_bad) HMSG_REQUIRE(why.empty(), HMSG_ERR_INVALID, "hmsg_graph_goal_views: " + why);
            } else {
                for (int r : g->floors[(size_t)f].rooms) HMSG_REQUIRE(g->goal_bad[(size_t)r].empty(), HMSG_ERR_INVALID, "hmsg_graph_goal_views: " + g->goal_bad[(size_t)r]);
            }
        }
        hmsg_goal_table_topk(t, Q, T, floor_id, k, (long long*)out_img, out_room, out_score, out_n);
    });
}

/* graph.py:2962-2986 for Q (text row, view) pairs, then visualize_pcd_on_image's avg_distance (:2994-2996) of the chosen object */
int hmsg_graph_rematch_in_views(hmsg_graph_t* g, int32_t Q, const float* T, const int32_t* view, const double* pose_inv, const int32_t* wh,
                                const double* K, int32_t* out_obj, double* out_score, double* out_avg_distance) {
    if (!g) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g->err, -1, [&] {
        views_ready(g, "hmsg_graph_rematch_in_views");
        HMSG_REQUIRE(Q >= 0 && (Q == 0 || (T && view && out_obj && out_score)) && (!pose_inv || (wh && K && out_avg_distance)), HMSG_ERR_INVALID,
                     "hmsg_graph_rematch_in_views: bad argument");
        if (Q == 0) return;
        for (int q = 0; q < Q; ++q)
            HMSG_REQUIRE(view[q] >= 0 && view[q] < (int32_t)g->views.size(), HMSG_ERR_INVALID, "hmsg_graph_rematch_in_views: view index out of range");
        int nfr = 0;
        hmsg_index_t* ix = hmsg_graph_shard_index(g, &nfr);
        if (!g->views_on_index) {
            const auto& lists = g->view_lists;
            std::vector<int64_t> off(1, 0);
            std::vector<int32_t> flat;
            for (auto& l : lists) {
                flat.insert(flat.end(), l.begin(), l.end());
                off.push_back((int64_t)flat.size());
            }
            const int rc = hmsg_index_set_views(ix, (int64_t)lists.size(), off.data(), flat.data());
            if (rc != HMSG_OK) throw hmsg_error{rc, hmsg_index_last_error(ix)};
            g->views_on_index = true;
        }
        std::vector<int32_t> h_obj((size_t)Q);
        const int rc = hmsg_rematch_in_views(ix, Q, T, view, h_obj.data(), out_score);
        if (rc != HMSG_OK) throw hmsg_error{rc, hmsg_index_last_error(ix)};
        if (pose_inv) {
            std::vector<long long> seg_off;
            std::vector<CloudSeg> segs;
            hipStream_t s = view_stream(g);
            const double* base = object_clouds(g, s, Q, h_obj.data(), seg_off, segs);
            hmsg_view_depths(s, base, Q, seg_off, segs, pose_inv, wh, K, g->prm.min_visible_ratio, g->prm.max_view_depth, out_avg_distance, nullptr,
                             nullptr);
        }
        write_out(out_obj, h_obj.data(), (size_t)Q * 4);
    });
}

/* graph.py:3011-3022: check_object_in_view(..., return_depth=True) of (object, camera) pairs */
int hmsg_graph_object_view_depths(hmsg_graph_t* g, int32_t n, const int32_t* obj, const double* view_pose_inv, const int32_t* wh, const double* K,
                                  uint8_t* visible, double* mean_depth) {
    if (!g) return HMSG_ERR_INVALID;
    return hmsg_boundary(&g->err, -1, [&] {
        views_ready(g, "hmsg_graph_object_view_depths");
        HMSG_REQUIRE(n >= 0 && (n == 0 || (obj && view_pose_inv && wh && K && visible && mean_depth)), HMSG_ERR_INVALID,
                     "hmsg_graph_object_view_depths: bad argument");
        if (n == 0) return;
        for (int i = 0; i < n; ++i)
            HMSG_REQUIRE(obj[i] >= 0 && obj[i] < (int32_t)g->objects.size(), HMSG_ERR_INVALID, "hmsg_graph_object_view_depths: object index out of range");
        hipStream_t s = view_stream(g);
        std::vector<long long> seg_off;
        std::vector<CloudSeg> segs;
        const double* base = object_clouds(g, s, n, obj, seg_off, segs);
        hmsg_view_depths(s, base, n, seg_off, segs, view_pose_inv, wh, K, g->prm.min_visible_ratio, g->prm.max_view_depth, nullptr, visible, mean_depth);
    });
}

}  // extern "C"
