// Stand-alone checks of the host side of the essential-graph optimisation:
// the planner (orb_slam_amd/csrc/orbx_essgraph_host.h) and the adapter's
// edge-list builder (orb_slam_amd/adapters/orbx_adapters.hpp,
// EssentialGraph::BuildEdges, the rules of src/Optimizer.cc:604-729).  Built
// with AddressSanitizer and UndefinedBehaviorSanitizer and run directly by
// tests/test_essgraph_plan.py; no GPU and no library.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbx_essgraph_host.h"
#include "../orb_slam_amd/adapters/orbx_adapters.hpp"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

using namespace orbx;
using ORB_SLAM_AMD::EssentialGraph;

static void plan_checks()
{
    // ids out of order, index 3 (id 3) fixed, index 5 (id 4) without an edge
    const int64_t ids[6] = {5, 1, 9, 3, 7, 4};
    const std::vector<orbx_essgraph_edge> e = {{0, 3, 0}, {0, 1, 1}, {4, 0, 1}, {2, 4, 1}, {2, 1, 1}, {1, 3, 1}, {2, 4, 1}};
    CHECK(essgraph_check(6, ids, 3, (int)e.size(), e.data()) == ORBX_OK);
    const EssPlan P = essgraph_plan(6, ids, 3, (int)e.size(), e.data());
    CHECK(P.n_free == 4);
    const int32_t want_free[6] = {1, 0, 3, -1, 2, -1};   // by id: 1, 5, 7, 9
    for (int k = 0; k < 6; k++) CHECK(P.free_of_kf[k] == want_free[k]);
    const int32_t want_kf[4] = {1, 0, 4, 2};
    for (int r = 0; r < 4; r++) CHECK(P.kf_of_free[r] == want_kf[r]);
    // rows: 0 alone; 1 - 0; 2 - 1; 3 - 0 (the long row: 9 - 1) and 3 - 2
    const int32_t want_first[4] = {0, 0, 1, 0};
    const int64_t want_off[5] = {0, 1, 3, 5, 9};
    for (int r = 0; r < 4; r++) CHECK(P.first[r] == want_first[r]);
    for (int r = 0; r <= 4; r++) CHECK(P.row_off[r] == want_off[r]);
    CHECK(P.n_blocks == 9 && P.max_row_blocks == 4);
    // columns: 0 <- rows 1, 3; 1 <- rows 2, 3 (fill: 9 - 5 has no edge); 2 <- row 3
    const int64_t want_col[5] = {0, 2, 4, 5, 5};
    const int32_t want_rows[5] = {1, 3, 2, 3, 3};
    for (int c = 0; c <= 4; c++) CHECK(P.col_off[c] == want_col[c]);
    for (int k = 0; k < 5; k++) CHECK(P.col_rows[k] == want_rows[k]);
    CHECK((long long)P.col_rows.size() == P.n_blocks - P.n_free);
    // incidence in edge order: free 0 (index 1): edges 1 (j), 4 (j), 5 (i)
    CHECK(P.inc_off[0] == 0 && P.inc_off[1] == 3);
    CHECK(P.inc_edge[0] == (1 << 1 | 1) && P.inc_edge[1] == (4 << 1 | 1) && P.inc_edge[2] == (5 << 1));
    // free 3 (index 2): edges 3, 4, 6 as i
    CHECK(P.inc_off[4] - P.inc_off[3] == 3 && P.inc_edge[P.inc_off[3]] == 3 << 1 && P.inc_edge[P.inc_off[3] + 2] == 6 << 1);
    CHECK(P.inc_off[4] == 12);   // 2 x 7 edge ends less the two on the fixed vertex
    CHECK(essgraph_blocks(6, ids, 3, (int)e.size(), e.data()) == 9);
    // no fixed vertex, no edge
    const EssPlan E = essgraph_plan(6, ids, -1, 0, nullptr);
    CHECK(E.n_free == 0 && E.n_blocks == 0 && E.max_row_blocks == 0 && E.row_off.size() == 1);
    // refused graphs
    const int64_t dup[3] = {4, 2, 4};
    const orbx_essgraph_edge ok01 = {0, 1, 1}, self = {1, 1, 1}, far = {0, 3, 1}, neg = {-1, 0, 0}, kind2 = {0, 1, 2};
    CHECK(essgraph_check(3, dup, 0, 1, &ok01) == ORBX_ERR_ARG);
    CHECK(essgraph_check(3, ids, 0, 1, &ok01) == ORBX_OK);
    CHECK(essgraph_check(3, ids, 0, 1, &self) == ORBX_ERR_ARG);
    CHECK(essgraph_check(3, ids, 0, 1, &far) == ORBX_ERR_ARG);
    CHECK(essgraph_check(3, ids, 0, 1, &neg) == ORBX_ERR_ARG);
    CHECK(essgraph_check(3, ids, 0, 1, &kind2) == ORBX_ERR_ARG);
    CHECK(essgraph_check(3, ids, 3, 1, &ok01) == ORBX_ERR_ARG);
    CHECK(essgraph_check(3, ids, -2, 1, &ok01) == ORBX_ERR_ARG);
    CHECK(essgraph_check(-1, ids, 0, 0, nullptr) == ORBX_ERR_ARG);
    CHECK(essgraph_check(3, ids, 0, 1, nullptr) == ORBX_ERR_ARG);
}

static bool has_edge(const std::vector<orbx_essgraph_edge>& e, int i, int j, int kind)
{
    for (const orbx_essgraph_edge& x : e)
        if (x.i == i && x.j == j && x.kind == kind) return true;
    return false;
}

static void edge_rule_checks()
{
    // keyframes (index: id): 0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5; loop keyframe 1, current keyframe 5.
    EssentialGraph G;
    for (unsigned long id = 0; id < 6; id++) {
        EssentialGraph::KeyFrame kf;
        kf.mnId = id;
        if (id > 0) kf.parent = (long long)id - 1;
        if (id < 5) kf.children = {id + 1};
        G.keyframes.push_back(kf);
    }
    G.loopKF = 1;
    G.curKF = 5;
    // (5, 1): weight below minFeat but exempt; (5, 2): below minFeat, dropped; (5, 0): kept; (4, 1): below
    // minFeat and not the (cur, loop) pair, dropped; (4, 2): kept and marks the pair (2, 4) inserted
    G.loopConnections = {{5, {{1, 20}, {2, 99}, {0, 100}}}, {4, {{1, 99}, {2, 150}}}};
    G.keyframes[3].loopEdges = {0, 4};          // 0 is smaller: an edge; 4 is larger: its own side adds it
    G.keyframes[4].loopEdges = {3};
    G.keyframes[4].covisibles = {3, 5, 2, 1, 0, 77};   // parent; child; inserted pair; a plain one; a plain one; not in the map
    G.keyframes[3].covisibles = {0, 1, 5};             // loop edge: excluded; plain; larger id: the other side's
    G.keyframes[5].covisibles = {3};                   // plain
    G.keyframes[1].covisibles = {4};                   // larger id only: nothing
    const std::vector<orbx_essgraph_edge> e = G.BuildEdges();
    const orbx_essgraph_edge want[] = {
        {5, 1, 0}, {5, 0, 0}, {4, 2, 0},          // the loop connections, in the caller's order
        {1, 0, 1},                                // keyframe 1: the parent
        {2, 1, 1},
        {3, 2, 1}, {3, 0, 1}, {3, 1, 1},          // parent, loop edge to the smaller id, covisible 1
        {4, 3, 1}, {4, 3, 1}, {4, 1, 1}, {4, 0, 1},   // parent, loop edge 3, covisibles 1 and 0
        {5, 4, 1}, {5, 3, 1},
    };
    CHECK(e.size() == sizeof(want) / sizeof(want[0]));
    for (size_t k = 0; k < e.size(); k++) CHECK(e[k].i == want[k].i && e[k].j == want[k].j && e[k].kind == want[k].kind);
    CHECK(!has_edge(e, 5, 2, 0) && !has_edge(e, 4, 1, 0));     // minFeat
    CHECK(!has_edge(e, 4, 2, 1));                              // sInsertedEdges
    CHECK(!has_edge(e, 4, 5, 1) && !has_edge(e, 3, 5, 1) && !has_edge(e, 1, 4, 1));   // child, smaller-id rule
    CHECK(!has_edge(e, 3, 4, 1));                              // a loop edge onto a larger id
    // the planner takes the adapter's edges
    std::vector<int64_t> ids;
    for (const EssentialGraph::KeyFrame& kf : G.keyframes) ids.push_back((int64_t)kf.mnId);
    CHECK(essgraph_check(6, ids.data(), G.IndexOf(G.loopKF), (int)e.size(), e.data()) == ORBX_OK);
    const EssPlan P = essgraph_plan(6, ids.data(), G.IndexOf(G.loopKF), (int)e.size(), e.data());
    CHECK(P.n_free == 5 && P.free_of_kf[1] == -1);
    // an id the map does not hold
    G.keyframes[2].parent = 42;
    bool thrown = false;
    try {
        G.BuildEdges();
    } catch (const ORB_SLAM_AMD::orbx_error& err) {
        thrown = err.code == ORBX_ERR_ARG;
    }
    CHECK(thrown);
}

int main()
{
    plan_checks();
    edge_rule_checks();
    std::printf("essgraph_check: ok\n");
    return 0;
}
