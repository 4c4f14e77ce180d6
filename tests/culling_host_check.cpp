// Stand-alone check of the culling additions to orbx_covis_host.h: the
// octave flags, the argument checks of the two cull calls, the shadow after a
// cull record (rows gone, observers in step, points erased), all-or-none on a
// capacity error, and the layout of orbx_covis_cull_args as the Python binding
// mirrors it.  Built with -fsanitize=address,undefined by
// tests/test_culling_host.py and run with nothing preloaded and no GPU.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbx_covis_host.h"

using namespace orbx;

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

static bool row_is(const CovisTable& t, int id, std::vector<int32_t> want) { return t.rows[(size_t)id] == want; }

// obs[p] names exactly the cells of the rows that hold p
static bool observers_match_rows(const CovisTable& t)
{
    size_t cells = 0, listed = 0;
    for (int id = 0; id < t.kf_capacity; id++) {
        const std::vector<int32_t>& row = t.rows[(size_t)id];
        if (!t.is_member(id) && !row.empty()) return false;
        for (size_t i = 0; i < row.size(); i++) {
            if (row[i] < 0) continue;
            cells++;
            bool found = false;
            for (uint32_t c : t.obs[(size_t)row[i]]) found = found || c == CovisTable::cell(id, (int)i);
            if (!found) return false;
        }
    }
    for (const auto& o : t.obs) listed += o.size();
    return cells == listed;
}

int main()
{
    CHECK(sizeof(orbx_covis_cull_args) == 80);
    CHECK(offsetof(orbx_covis_cull_args, cur) == 0 && offsetof(orbx_covis_cull_args, n_keep) == 4);
    CHECK(offsetof(orbx_covis_cull_args, keep) == 8 && offsetof(orbx_covis_cull_args, max_culls) == 16);
    CHECK(offsetof(orbx_covis_cull_args, cand_cap) == 20 && offsetof(orbx_covis_cull_args, cand) == 24);
    CHECK(offsetof(orbx_covis_cull_args, n_cand) == 32 && offsetof(orbx_covis_cull_args, n_done) == 36);
    CHECK(offsetof(orbx_covis_cull_args, n_mps) == 40 && offsetof(orbx_covis_cull_args, n_redundant) == 48);
    CHECK(offsetof(orbx_covis_cull_args, decision) == 56 && offsetof(orbx_covis_cull_args, bad_points) == 64);
    CHECK(offsetof(orbx_covis_cull_args, bad_cap) == 72 && offsetof(orbx_covis_cull_args, n_bad) == 76);

    CovisTable t;
    CHECK(t.create(8, 40, 5) == ORBX_OK);
    // point 10 in 1, 2, 3, 4; 11 in 1, 2, 5; 12 in 1 alone
    const int32_t r1[] = {10, 11, 12}, r2[] = {11, -1, 10}, r3[] = {10}, r4[] = {-1, 10}, r5[] = {11};
    t.commit_add(1, 100, 3, r1);
    t.commit_add(2, 200, 3, r2);
    t.commit_add(3, 300, 1, r3);
    t.commit_add(4, 400, 2, r4);
    t.commit_add(5, 500, 1, r5);
    CHECK(t.member_cells() == 10 && observers_match_rows(t));

    // octave flags: a member, the row's length, a pointer
    const uint8_t o3[] = {0, 1, 2};
    CHECK(t.check_octaves(0, 0, nullptr) == ORBX_ERR_ARG);    // not a member
    CHECK(t.check_octaves(8, 3, o3) == ORBX_ERR_ARG);
    CHECK(t.check_octaves(1, 2, o3) == ORBX_ERR_ARG);         // another n
    CHECK(t.check_octaves(1, 3, nullptr) == ORBX_ERR_ARG);
    CHECK(t.check_octaves(1, 3, o3) == ORBX_OK);
    CHECK(!t.has_octaves(1) && !t.every_member_has_octaves());

    // the cull call's arguments
    int32_t cand[8] = {1, 2, 7, 1}, mps[8], red[8], dec[8], bad[8], keep[2] = {2, 8};
    orbx_covis_cull_args q{};
    q.cur = -1;
    q.cand = cand;
    q.n_cand = 4;
    q.cand_cap = 8;
    q.n_mps = mps;
    q.n_redundant = red;
    q.decision = dec;
    q.bad_points = bad;
    q.bad_cap = 8;
    CHECK(t.check_cull(nullptr) == ORBX_ERR_ARG);
    CHECK(t.check_cull(&q) == ORBX_ERR_ARG);                  // no member has octaves yet
    for (int id = 1; id <= 5; id++) t.commit_octaves(id);
    CHECK(t.has_octaves(1) && t.every_member_has_octaves());
    CHECK(t.check_cull(&q) == ORBX_OK);                       // 7 was never added, 1 stands twice: no error
    q.n_keep = 2;
    q.keep = keep;
    CHECK(t.check_cull(&q) == ORBX_ERR_ARG);                  // kept id 8 out of range
    q.n_keep = 1;
    CHECK(t.check_cull(&q) == ORBX_OK);
    q.keep = nullptr;
    CHECK(t.check_cull(&q) == ORBX_ERR_ARG);
    q.n_keep = 0;
    cand[2] = 8;
    CHECK(t.check_cull(&q) == ORBX_ERR_ARG);                  // listed id out of range
    cand[2] = -1;
    CHECK(t.check_cull(&q) == ORBX_ERR_ARG);
    cand[2] = 7;
    q.max_culls = -1;
    CHECK(t.check_cull(&q) == ORBX_ERR_ARG);
    q.max_culls = 0;
    q.cand_cap = 3;
    CHECK(t.check_cull(&q) == ORBX_ERR_CAPACITY);             // the caller's own list does not fit
    q.cand_cap = 8;
    q.n_cand = 9;
    CHECK(t.check_cull(&q) == ORBX_ERR_ARG);                  // longer than kf_capacity
    q.n_cand = 4;
    q.decision = nullptr;
    CHECK(t.check_cull(&q) == ORBX_ERR_ARG);
    q.decision = dec;
    q.bad_cap = -1;
    CHECK(t.check_cull(&q) == ORBX_ERR_ARG);
    q.bad_cap = 8;
    q.cur = 6;
    CHECK(t.check_cull(&q) == ORBX_ERR_ARG);                  // cur no member
    q.cur = -2;
    CHECK(t.check_cull(&q) == ORBX_ERR_ARG);
    q.cur = 3;
    CHECK(t.check_cull(&q) == ORBX_OK);

    // a cull record: keyframe 1 went, which left 11 with two observers and 12 with none
    const int32_t c2[] = {0, 1, 2}, d2[] = {-1, 1, 0}, b2[] = {11, 12};
    CHECK(t.apply_cull(3, 2, 3, c2, d2, 2, 8, b2) == ORBX_ERR_CAPACITY);   // n_cand above its capacity: no change
    CHECK(t.apply_cull(3, 8, 3, c2, d2, 2, 1, b2) == ORBX_ERR_CAPACITY);   // n_bad above its capacity: no change
    CHECK(t.size == 5 && row_is(t, 1, {10, 11, 12}) && !t.erased[11] && observers_match_rows(t));
    const int32_t far[] = {11, 40}, d3[] = {1, 1, 0};
    CHECK(t.apply_cull(3, 8, 3, c2, d2, 2, 8, far) == ORBX_ERR_ARG);       // a point out of range: no change
    CHECK(t.apply_cull(3, 8, 3, c2, d3, 2, 8, b2) == ORBX_ERR_ARG);        // a culled keyframe that is no member
    CHECK(t.apply_cull(3, 8, 4, c2, d2, 2, 8, b2) == ORBX_ERR_ARG);        // n_done above n_cand
    CHECK(t.size == 5 && row_is(t, 1, {10, 11, 12}) && !t.erased[11] && observers_match_rows(t));
    CHECK(t.apply_cull(3, 8, 3, c2, d2, 2, 8, b2) == ORBX_OK);
    CHECK(t.size == 4 && !t.is_member(1) && t.rows[1].empty() && t.erased[11] && t.erased[12] && !t.erased[10]);
    CHECK(row_is(t, 2, {-1, -1, 10}) && row_is(t, 5, {-1}) && row_is(t, 3, {10}) && observers_match_rows(t));
    CHECK(t.obs[11].empty() && t.obs[12].empty() && t.obs[10].size() == 3 && t.member_cells() == 7);
    // only the first n_done decisions count
    const int32_t d4[] = {0, 1};
    const int32_t c4[] = {2, 3};
    CHECK(t.apply_cull(2, 8, 1, c4, d4, 0, 8, nullptr) == ORBX_OK && t.is_member(3));
    CHECK(t.check_add(1, 900, 1, r3) == ORBX_ERR_ARG);                     // a culled id is never reused

    // MapPointCulling's arguments and its record
    const int32_t ids[] = {10, 20, 30}, fv[] = {1, 1, 1}, first[] = {5, 7, 6}, twice[] = {10, 20, 10}, out[] = {10, 40, 30};
    const int32_t neg[] = {1, -1, 1}, late[] = {5, 8, 6};
    int32_t act[3] = {0, 0, 0};
    CHECK(t.check_cull_points(7, 3, ids, fv, fv, first, act) == ORBX_OK);
    CHECK(t.check_cull_points(7, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == ORBX_OK);
    CHECK(t.check_cull_points(7, -1, ids, fv, fv, first, act) == ORBX_ERR_ARG);
    CHECK(t.check_cull_points(7, 3, twice, fv, fv, first, act) == ORBX_ERR_ARG);   // listed twice
    CHECK(t.check_cull_points(7, 3, out, fv, fv, first, act) == ORBX_ERR_ARG);     // out of range
    CHECK(t.check_cull_points(7, 3, ids, neg, fv, first, act) == ORBX_ERR_ARG);    // a negative count
    CHECK(t.check_cull_points(7, 3, ids, fv, neg, first, act) == ORBX_ERR_ARG);
    CHECK(t.check_cull_points(7, 3, ids, fv, fv, late, act) == ORBX_ERR_ARG);      // first_kf > cur_kf
    CHECK(t.check_cull_points(7, 3, ids, fv, fv, neg, act) == ORBX_ERR_ARG);
    CHECK(t.check_cull_points(7, 3, ids, fv, nullptr, first, act) == ORBX_ERR_ARG);
    CHECK(t.check_cull_points(-1, 3, ids, fv, fv, first, act) == ORBX_ERR_ARG);
    const int32_t a1[] = {3, 4, 2};
    t.apply_cull_points(3, ids, a1);                                       // 10 and 30 go, 20 only leaves the list
    CHECK(t.erased[10] && t.erased[30] && !t.erased[20] && row_is(t, 2, {-1, -1, -1}) && row_is(t, 3, {-1}));
    CHECK(observers_match_rows(t) && t.member_cells() == 7);

    // clear takes the octave flags with it
    t.clear();
    CHECK(t.check_add(1, 100, 3, r1) == ORBX_OK);
    t.commit_add(1, 100, 3, r1);
    CHECK(!t.has_octaves(1) && !t.every_member_has_octaves());
    std::puts("culling host bookkeeping: ok");
    return 0;
}
