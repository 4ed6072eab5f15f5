// Random merge fold histories through the host planner of holoagent_amd/csrc/hmsg_fold_host.h (tests/test_fold_host_plan.py builds
// and runs this program, once plain and once with -fsanitize=address,undefined).
//
// A history is 1-40 fold steps over a list of at most 60 clouds.  Every step the list is [what the last step put out | a frame's
// masks]; pairs that pass the box test are united at random into components, components become DBSCAN segments by the fold's own
// rule, and the "results" of the segments are drawn at random: a single cloud comes through unchanged or changed, a merged one is
// always new; either may come out empty.  After every step
//   * FoldPlan's pair list (ahead part + late part, or the reference enumerator on the kept table) must equal, in content and
//     order, the list of fold_pairs_reference on a table filled from the cloud list;
//   * the kept box table must equal that freshly filled table;
//   * the cloud list updated in place must equal the list rebuilt by copying.
// Boxes come from a coarse lattice so that they touch, nest and coincide all the time; some have no extent on an axis; some
// clouds are empty; frames may have no masks; the next frame is sometimes unknown when a step plans ahead (and always at a
// history's last step), and sometimes the ahead part is dropped afterwards (what a collection of the pool does).
#include "hmsg_fold_host.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>

namespace {

struct Cloud {
    double mn[3], mx[3];
    int n;
    bool fresh, fixed;
    int tag;        // identity, to tell clouds with equal boxes apart
};
bool same_cloud(const Cloud& a, const Cloud& b) {
    for (int k = 0; k < 3; ++k)
        if (a.mn[k] != b.mn[k] || a.mx[k] != b.mx[k]) return false;
    return a.n == b.n && a.fresh == b.fresh && a.fixed == b.fixed && a.tag == b.tag;
}

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    int below(int n) { return (int)(next() % (uint32_t)n); }
    bool chance(int percent) { return below(100) < percent; }
};

int g_tag = 0;
Cloud random_cloud(Rng& r, bool may_be_empty) {
    Cloud c;
    for (int k = 0; k < 3; ++k) {
        const int a = r.below(7), len = r.chance(8) ? 0 : 1 + r.below(4);   // (8 %: no extent on this axis)
        c.mn[k] = 0.5 * a;
        c.mx[k] = 0.5 * (a + len);
    }
    c.n = (may_be_empty && r.chance(10)) ? 0 : 1 + r.below(50);
    c.fresh = true;
    c.fixed = false;
    c.tag = ++g_tag;
    return c;
}

struct Coverage {
    long steps = 0, ahead_steps = 0, late_only_steps = 0, pairs = 0, changed = 0, unchanged = 0, absorbed_far = 0, no_masks = 0,
         next_absent = 0, dropped = 0, empty_out = 0, degenerate = 0;
};

#define REQUIRE(cond, ...)                          \
    do {                                            \
        if (!(cond)) {                              \
            fprintf(stderr, "FAILED: " __VA_ARGS__); \
            fprintf(stderr, "\n");                  \
            return false;                           \
        }                                           \
    } while (0)

bool run_history(uint64_t seed, Coverage& cov) {
    Rng r{seed * 0x9E3779B97F4A7C15ull + 12345};
    const int steps = 1 + r.below(40);
    const double th = r.chance(20) ? 0.0 : 0.05;
    const int unite_percent = 10 + r.below(60);
    FoldPlan plan;
    FoldBoxTable ref_tab;
    FoldPairScratch ref_scratch;
    FoldPairList got, want;
    std::vector<Cloud> L, L_rebuilt;          // the list updated in place / rebuilt per step
    auto draw_frame = [&](size_t room) {
        std::vector<Cloud> f;
        const int nm = r.chance(12) ? 0 : r.below((int)std::min<size_t>(room, 8) + 1);
        for (int k = 0; k < nm; ++k) f.push_back(random_cloud(r, true));
        return f;
    };
    std::vector<Cloud> frame = draw_frame(60);
    for (int st = 0; st < steps; ++st) {
        cov.steps += 1;
        if (frame.empty()) cov.no_masks += 1;
        L.insert(L.end(), frame.begin(), frame.end());
        L_rebuilt.insert(L_rebuilt.end(), frame.begin(), frame.end());
        const int n = (int)L.size();
        // ---- pairs: planner against reference
        got.clear();
        const double ahead_before = plan.n_ahead_steps;
        plan.step_pairs(L, th, got);
        (plan.n_ahead_steps > ahead_before ? cov.ahead_steps : cov.late_only_steps) += 1;
        fold_fill_boxes(L_rebuilt, 0, ref_tab);
        want.clear();
        fold_pairs_reference(ref_tab, th, ref_scratch, want);
        REQUIRE(plan.tab.n == n, "seed %llu step %d: table has %d entries, list %d", (unsigned long long)seed, st, plan.tab.n, n);
        for (int i = 0; i < n; ++i)
            REQUIRE(plan.tab.same(i, ref_tab, i), "seed %llu step %d: kept table entry %d differs", (unsigned long long)seed, st, i);
        REQUIRE(got.size() == want.size(), "seed %llu step %d: %zu pairs, reference %zu", (unsigned long long)seed, st, got.size(), want.size());
        for (size_t k = 0; k < got.size(); ++k)
            REQUIRE(got[k] == want[k], "seed %llu step %d: pair %zu is (%d, %d), reference (%d, %d)", (unsigned long long)seed, st, k,
                    got[k].first, got[k].second, want[k].first, want[k].second);
        cov.pairs += (long)got.size();
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) {
                if (L[(size_t)i].n && L[(size_t)i].mn[k] == L[(size_t)i].mx[k]) cov.degenerate += 1;
            }
        // ---- components: lowest member labels, in order of the lowest member (scipy connected_components)
        std::vector<int> parent((size_t)n);
        std::iota(parent.begin(), parent.end(), 0);
        auto find = [&](int x) {
            while (parent[(size_t)x] != x) x = parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
            return x;
        };
        for (auto& p : got)
            if (r.chance(unite_percent)) {
                const int a = find(p.first), b = find(p.second);
                if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);
            }
        std::vector<int> comp_of((size_t)n, -1), cid((size_t)n), off, mem((size_t)n);
        int nc = 0;
        for (int i = 0; i < n; ++i) {
            const int root = find(i);
            if (comp_of[(size_t)root] < 0) comp_of[(size_t)root] = nc++;
            cid[(size_t)i] = comp_of[(size_t)root];
        }
        off.assign((size_t)nc + 1, 0);
        for (int i = 0; i < n; ++i) ++off[(size_t)cid[(size_t)i] + 1];
        for (int c = 0; c < nc; ++c) off[(size_t)c + 1] += off[(size_t)c];
        {
            std::vector<int> cur(off.begin(), off.end() - 1);
            for (int i = 0; i < n; ++i) mem[(size_t)cur[(size_t)cid[(size_t)i]]++] = i;
        }
        // segments: every component but a single cloud that is fixed or empty
        std::vector<int> seg_of_comp((size_t)nc, -1);
        int nseg = 0;
        for (int c = 0; c < nc; ++c) {
            const int m0 = mem[(size_t)off[(size_t)c]], sz = off[(size_t)c + 1] - off[(size_t)c];
            if (sz == 1 && (L[(size_t)m0].fixed || L[(size_t)m0].n == 0)) continue;
            seg_of_comp[(size_t)c] = nseg++;
            if (sz > 1 && mem[(size_t)off[(size_t)c + 1] - 1] - m0 > sz) cov.absorbed_far += 1;     // members not next to each other
        }
        // ---- behind the batch's publish: the table moves on, the next frame's masks (if known) are planned ahead
        const bool last = st + 1 == steps;
        std::vector<Cloud> next = last ? std::vector<Cloud>() : draw_frame((size_t)std::max(0, 60 - nc));
        const bool next_known = !last && !r.chance(20);
        if (!next_known) cov.next_absent += 1;
        plan.advance(off.data(), mem.data(), nc, seg_of_comp.data());
        if (next_known) {
            for (auto& c : next) plan.append(c.mn, c.mx, c.n);
            plan.plan_ahead(th);
        }
        // ---- the results, entered into both lists
        std::vector<Cloud> out;
        for (int c = 0; c < nc; ++c) {
            const int m0 = mem[(size_t)off[(size_t)c]], sz = off[(size_t)c + 1] - off[(size_t)c];
            if (seg_of_comp[(size_t)c] < 0) {
                Cloud k = L_rebuilt[(size_t)m0];
                k.fresh = false;
                k.fixed = true;
                out.push_back(k);
                fold_keep_untouched(L, (size_t)c, (size_t)m0);
                continue;
            }
            Cloud k = L_rebuilt[(size_t)m0];
            int total = 0;
            for (int q = off[(size_t)c]; q < off[(size_t)c + 1]; ++q) {        // the members' common box
                const Cloud& mcl = L_rebuilt[(size_t)mem[(size_t)q]];
                if (!mcl.n) continue;
                for (int a = 0; a < 3; ++a) {
                    k.mn[a] = total ? std::min(k.mn[a], mcl.mn[a]) : mcl.mn[a];
                    k.mx[a] = total ? std::max(k.mx[a], mcl.mx[a]) : mcl.mx[a];
                }
                total += mcl.n;
            }
            if (sz == 1 && r.chance(50)) {         // DBSCAN kept every point: the same cloud, now fixed
                k = L_rebuilt[(size_t)m0];
                k.fresh = false;
                k.fixed = true;
                cov.unchanged += 1;
            } else {                               // a new cloud: fewer points (none, sometimes), a box inside the members' box
                k.n = r.chance(10) ? 0 : (sz == 1 ? r.below(std::max(1, total)) : 1 + r.below(std::max(1, total)));
                for (int a = 0; a < 3; ++a)
                    if (r.chance(30) && k.mx[a] - k.mn[a] >= 1.0) {
                        if (r.chance(50)) k.mn[a] += 0.5;
                        else k.mx[a] -= 0.5;
                    }
                k.fresh = true;
                k.fixed = r.chance(60);
                k.tag = ++g_tag;
                cov.changed += 1;
                if (!k.n) cov.empty_out += 1;
            }
            out.push_back(k);
            L[(size_t)c] = k;
            plan.resolve(c, k.mn, k.mx, k.n, k.fresh);
        }
        L.resize((size_t)nc);
        L_rebuilt.swap(out);
        REQUIRE(plan.resolved(), "seed %llu step %d: outputs left unresolved", (unsigned long long)seed, st);
        REQUIRE(L.size() == L_rebuilt.size(), "seed %llu step %d: list lengths differ", (unsigned long long)seed, st);
        for (size_t i = 0; i < L.size(); ++i)
            REQUIRE(same_cloud(L[i], L_rebuilt[i]), "seed %llu step %d: in-place list differs from the rebuilt one at %zu", (unsigned long long)seed, st, i);
        if (next_known && r.chance(10)) {          // (a collection of the pool between two steps)
            plan.drop_ahead();
            cov.dropped += 1;
        }
        frame.swap(next);
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const long histories = argc > 1 ? atol(argv[1]) : 3000;
    Coverage cov;
    for (long h = 0; h < histories; ++h)
        if (!run_history((uint64_t)h, cov)) return 1;
    printf("histories %ld steps %ld ahead_steps %ld late_only_steps %ld pairs %ld changed %ld unchanged %ld absorbed_far %ld no_masks %ld "
           "next_absent %ld dropped %ld empty_out %ld degenerate %ld\n",
           histories, cov.steps, cov.ahead_steps, cov.late_only_steps, cov.pairs, cov.changed, cov.unchanged, cov.absorbed_far, cov.no_masks,
           cov.next_absent, cov.dropped, cov.empty_out, cov.degenerate);
    // every kind of step the histories are meant to cover has to have occurred
    const long need[] = {cov.ahead_steps, cov.late_only_steps, cov.pairs, cov.changed, cov.unchanged, cov.absorbed_far, cov.no_masks,
                         cov.next_absent, cov.dropped, cov.empty_out, cov.degenerate};
    for (long v : need)
        if (v <= 0) {
            fprintf(stderr, "FAILED: a kind of step never occurred\n");
            return 2;
        }
    return 0;
}
