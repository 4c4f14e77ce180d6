// Stand-alone check of orbx_covis_host.h (the covisibility map's host
// bookkeeping): built with -fsanitize=address,undefined by
// tests/test_covis_host.py and run with nothing preloaded and no GPU.
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
    // the C struct as the Python binding lays it out
    CHECK(sizeof(orbx_covis_reference_args) == 64);
    CHECK(offsetof(orbx_covis_reference_args, frame_mp) == 8 && offsetof(orbx_covis_reference_args, local_kf) == 24);
    CHECK(offsetof(orbx_covis_reference_args, ref_kf) == 44 && offsetof(orbx_covis_reference_args, local_mp) == 48);
    CHECK(offsetof(orbx_covis_reference_args, n_local_mp) == 60);

    // creation bounds
    CHECK(CovisTable::check_create(0, 10, 10) == ORBX_ERR_ARG);
    CHECK(CovisTable::check_create(10, 0, 10) == ORBX_ERR_ARG);
    CHECK(CovisTable::check_create(10, 10, 0) == ORBX_ERR_ARG);
    CHECK(CovisTable::check_create(kCovisMaxKeyframes, 10, kCovisMaxKeypoints) == ORBX_OK);
    CHECK(CovisTable::check_create(kCovisMaxKeyframes + 1, 10, 10) == ORBX_ERR_UNSUPPORTED);
    CHECK(CovisTable::check_create(10, 10, kCovisMaxKeypoints + 1) == ORBX_ERR_UNSUPPORTED);
    CHECK(CovisTable::check_create(10, kCovisMaxPoints + 1, 10) == ORBX_ERR_UNSUPPORTED);
    CHECK(kCovisMaxKeyframes == 8192 && kCovisMaxKeypoints == 65535);
    // a cell holds the largest id and index
    CHECK(CovisTable::cell_kf(CovisTable::cell(8191, 65534)) == 8191 && CovisTable::cell_idx(CovisTable::cell(8191, 65534)) == 65534);

    CovisTable t;
    CHECK(t.create(8, 20, 5) == ORBX_OK);
    CHECK(t.size == 0 && t.hi == 0);

    // the id table, the rows' checks
    const int32_t r3[] = {4, -1, 7, 9}, dup[] = {4, 5, 4}, big[] = {20}, low[] = {-2}, six[] = {1, 2, 3, 4, 5, 6};
    CHECK(t.check_add(-1, 100, 4, r3) == ORBX_ERR_ARG);
    CHECK(t.check_add(8, 100, 4, r3) == ORBX_ERR_ARG);
    CHECK(t.check_add(3, 100, 3, dup) == ORBX_ERR_ARG);    // a point twice
    CHECK(t.check_add(3, 100, 1, big) == ORBX_ERR_ARG);    // point id out of range
    CHECK(t.check_add(3, 100, 1, low) == ORBX_ERR_ARG);
    CHECK(t.check_add(3, 100, 6, six) == ORBX_ERR_ARG);    // longer than max_keypoints
    CHECK(t.check_add(3, 100, -1, r3) == ORBX_ERR_ARG);
    CHECK(t.check_add(3, 100, 2, nullptr) == ORBX_ERR_ARG);
    CHECK(t.check_add(3, 100, 0, nullptr) == ORBX_OK);     // an empty row
    CHECK(t.check_add(3, 100, 4, r3) == ORBX_OK);
    t.commit_add(3, 100, 4, r3);
    CHECK(t.size == 1 && t.hi == 4 && t.is_member(3) && row_is(t, 3, {4, -1, 7, 9}));
    CHECK(t.check_add(3, 101, 4, r3) == ORBX_ERR_ARG);     // in use
    // keys: distinct among all ever added; the full 64 bits order them
    CHECK(t.check_add(5, 100, 4, r3) == ORBX_ERR_ARG);
    const int32_t r5[] = {7, 4, 1}, r0[] = {9};
    t.commit_add(5, 0xF000000000000001ull, 3, r5);
    t.commit_add(0, 50, 1, r0);
    CHECK(t.size == 3 && t.hi == 6);
    CHECK(t.rank[0] == 0 && t.rank[3] == 1 && t.rank[5] == 2 && t.rank[1] == -1);
    CHECK(t.by_rank[0] == 0 && t.by_rank[1] == 3 && t.by_rank[2] == 5 && t.by_rank[3] == -1);
    const int32_t r6[] = {2};
    CHECK(t.check_add(6, 75, 1, r6) == ORBX_OK);
    t.commit_add(6, 75, 1, r6);                            // lands between: the ranks above move up
    CHECK(t.rank[0] == 0 && t.rank[6] == 1 && t.rank[3] == 2 && t.rank[5] == 3 && t.by_rank[3] == 5);
    CHECK(t.key_used(75) && t.key_used(0xF000000000000001ull) && !t.key_used(76));
    CHECK(t.in_row(3, 7) && t.in_row(5, 7) && !t.in_row(0, 7) && observers_match_rows(t));

    // edits on the shadow, in order, all or none
    const int32_t i0[] = {1}, p0[] = {7};
    CHECK(t.set_matches(3, 1, i0, p0) == ORBX_ERR_ARG);    // 7 stands at index 2
    const int32_t i1[] = {2, 1}, p1[] = {-1, 7};
    CHECK(t.set_matches(3, 2, i1, p1) == ORBX_OK);         // it leaves index 2 first
    CHECK(row_is(t, 3, {4, 7, -1, 9}) && observers_match_rows(t));
    const int32_t i2[] = {0, 2, 3}, p2[] = {11, 12, 7};
    CHECK(t.set_matches(3, 3, i2, p2) == ORBX_ERR_ARG);    // the third edit fails: the first two are undone
    CHECK(row_is(t, 3, {4, 7, -1, 9}) && observers_match_rows(t));
    const int32_t i3[] = {0, 0, 0}, p3[] = {11, 12, 20};
    CHECK(t.set_matches(3, 3, i3, p3) == ORBX_ERR_ARG);    // the same index twice, then a point out of range
    CHECK(row_is(t, 3, {4, 7, -1, 9}) && observers_match_rows(t));
    const int32_t i4[] = {4}, i5[] = {-1}, p4[] = {1};
    CHECK(t.set_matches(3, 1, i4, p4) == ORBX_ERR_ARG);    // index outside the row
    CHECK(t.set_matches(3, 1, i5, p4) == ORBX_ERR_ARG);
    CHECK(t.set_matches(1, 1, i0, p4) == ORBX_ERR_ARG);    // not a member
    CHECK(t.set_matches(3, 0, nullptr, nullptr) == ORBX_OK);
    const int32_t i6[] = {0, 0}, p6[] = {4, 13};
    CHECK(t.set_matches(3, 2, i6, p6) == ORBX_OK);         // writing the point that stands there is no duplicate
    CHECK(row_is(t, 3, {13, 7, -1, 9}) && !t.in_row(3, 4) && observers_match_rows(t));

    // erase_points: out of every row, with the cells named; erased ids stay usable in rows
    const int32_t bad[] = {7, 19}, out_of_range[] = {20};
    CHECK(t.check_points(1, out_of_range) == ORBX_ERR_ARG && t.check_points(2, bad) == ORBX_OK);
    std::vector<uint32_t> cells;
    t.erase_points(2, bad, cells);
    CHECK(cells.size() == 2 && t.erased[7] && t.erased[19] && !t.erased[4]);
    CHECK(row_is(t, 3, {13, -1, -1, 9}) && row_is(t, 5, {-1, 4, 1}) && observers_match_rows(t));
    CHECK(t.set_matches(5, 1, i5 + 0, p0) == ORBX_ERR_ARG);
    const int32_t i7[] = {0};
    CHECK(t.set_matches(5, 1, i7, p0) == ORBX_OK && row_is(t, 5, {7, 4, 1}));   // an erased point in a row: no error

    // erase a keyframe: its observations go, its id, key and rank stay taken
    CHECK(t.check_erase_keyframe(1) == ORBX_ERR_ARG && t.check_erase_keyframe(3) == ORBX_OK);
    t.commit_erase_keyframe(3);
    CHECK(!t.is_member(3) && t.size == 3 && t.hi == 7 && t.rank[3] == 2 && observers_match_rows(t));
    CHECK(!t.in_row(3, 9) && t.in_row(0, 9));
    CHECK(t.check_add(3, 500, 1, r0) == ORBX_ERR_ARG);     // never reused
    CHECK(t.check_add(1, 100, 1, r6) == ORBX_ERR_ARG);     // nor is its key
    const int32_t mem[] = {0, 5, 6}, gone[] = {0, 3};
    CHECK(t.check_members(3, mem) == ORBX_OK && t.check_members(2, gone) == ORBX_ERR_ARG);
    CHECK(t.check_members(1, nullptr) == ORBX_ERR_ARG && t.check_members(0, nullptr) == ORBX_OK);

    // frames: a point may stand twice
    const int32_t f[] = {4, 4, -1, 19};
    CHECK(t.frame_ok(4, f) && !t.frame_ok(1, big) && !t.frame_ok(6, six) && t.frame_ok(0, nullptr));

    // clear frees everything
    t.clear();
    CHECK(t.size == 0 && t.hi == 0 && !t.key_used(100) && !t.erased[7] && t.check_add(3, 100, 4, r3) == ORBX_OK);
    CHECK(covis_sort_len(0) == 2 && covis_sort_len(3) == 4 && covis_sort_len(64) == 64 && covis_sort_len(65) == 128);
    std::puts("covis host bookkeeping: ok");
    return 0;
}
