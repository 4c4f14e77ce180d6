// Stand-alone check of orbx_kfdb_host.h (the keyframe database's host
// bookkeeping): built with -fsanitize=address,undefined by
// tests/test_kfdb_host.py and run with nothing preloaded and no GPU.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbx_kfdb_host.h"

using namespace orbx;

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

int main()
{
    // the C struct as the Python binding lays it out
    CHECK(sizeof(orbx_kfdb_query_args) == 136);
    CHECK(offsetof(orbx_kfdb_query_args, words) == 16 && offsetof(orbx_kfdb_query_args, candidates) == 64);
    CHECK(offsetof(orbx_kfdb_query_args, tap_words) == 96);

    // creation bounds
    CHECK(KfdbTable::check_create(0, 10) == ORBX_ERR_ARG);
    CHECK(KfdbTable::check_create(10, 0) == ORBX_ERR_ARG);
    CHECK(KfdbTable::check_create(kKfdbMaxMembers, kKfdbMaxWords) == ORBX_OK);
    CHECK(KfdbTable::check_create(kKfdbMaxMembers + 1, 10) == ORBX_ERR_UNSUPPORTED);
    CHECK(KfdbTable::check_create(10, kKfdbMaxWords + 1) == ORBX_ERR_UNSUPPORTED);
    CHECK(kKfdbMaxMembers >= 8192);

    KfdbTable t;
    CHECK(t.create(8, 5) == ORBX_OK);
    CHECK(t.size == 0 && t.hi == 0);
    // ids
    CHECK(t.check_add(-1, 1) == ORBX_ERR_ARG);
    CHECK(t.check_add(8, 1) == ORBX_ERR_ARG);
    CHECK(t.check_add(3, 6) == ORBX_ERR_CAPACITY);
    CHECK(t.check_add(3, 5) == ORBX_OK);
    CHECK(t.check_add(3, 0) == ORBX_OK);
    CHECK(t.commit_add(3) == 0u);
    CHECK(t.size == 1 && t.hi == 4 && t.is_member(3));
    CHECK(t.check_add(3, 1) == ORBX_ERR_ARG);   // in use
    CHECK(t.commit_add(7) == 1u);
    CHECK(t.commit_add(0) == 2u);
    CHECK(t.size == 3 && t.hi == 8);
    // erase keeps the counter: an id added again goes to the back
    CHECK(t.check_erase(5) == ORBX_ERR_ARG);
    CHECK(t.check_erase(-3) == ORBX_ERR_ARG);
    CHECK(t.check_erase(7) == ORBX_OK);
    t.commit_erase(7);
    CHECK(!t.is_member(7) && t.size == 2 && t.hi == 8);
    CHECK(t.check_add(7, 2) == ORBX_OK);
    CHECK(t.commit_add(7) == 3u);
    // lists
    const int32_t good[] = {0, 3, 7}, stale[] = {0, 5}, out[] = {0, 8}, neg[] = {-1};
    CHECK(t.check_ids(3, good) == ORBX_OK && t.check_members(3, good) == ORBX_OK);
    CHECK(t.check_ids(2, stale) == ORBX_OK && t.check_members(2, stale) == ORBX_ERR_ARG);
    CHECK(t.check_ids(2, out) == ORBX_ERR_ARG && t.check_members(2, out) == ORBX_ERR_ARG);
    CHECK(t.check_ids(1, neg) == ORBX_ERR_ARG);
    CHECK(t.check_ids(0, nullptr) == ORBX_OK && t.check_ids(1, nullptr) == ORBX_ERR_ARG);
    CHECK(t.check_ids(-1, good) == ORBX_ERR_ARG);
    // counter exhaustion
    t.next_seq = UINT32_MAX;
    CHECK(t.check_add(1, 1) == ORBX_ERR_UNSUPPORTED);
    t.clear();
    CHECK(t.size == 0 && t.hi == 0 && t.next_seq == 0 && !t.is_member(3));
    CHECK(t.check_add(1, 1) == ORBX_OK);

    // BowVectors: strictly ascending words, finite values
    const uint32_t w_ok[] = {1, 5, 9}, w_dup[] = {1, 5, 5}, w_desc[] = {5, 1, 9};
    const double v_ok[] = {0.5, 0.25, 0.25}, v_nan[] = {0.5, NAN, 0.25}, v_inf[] = {INFINITY, 0.1, 0.2};
    CHECK(KfdbTable::bow_ok(3, w_ok, v_ok));
    CHECK(KfdbTable::bow_ok(0, nullptr, nullptr));
    CHECK(!KfdbTable::bow_ok(-1, w_ok, v_ok));
    CHECK(!KfdbTable::bow_ok(3, nullptr, v_ok) && !KfdbTable::bow_ok(3, w_ok, nullptr));
    CHECK(!KfdbTable::bow_ok(3, w_dup, v_ok) && !KfdbTable::bow_ok(3, w_desc, v_ok));
    CHECK(!KfdbTable::bow_ok(3, w_ok, v_nan) && !KfdbTable::bow_ok(3, w_ok, v_inf));

    // every id of a full table, on the heap so that the sanitizer sees an overrun
    KfdbTable full;
    CHECK(full.create(kKfdbMaxMembers, 1) == ORBX_OK);
    for (int i = kKfdbMaxMembers - 1; i >= 0; i--) {
        CHECK(full.check_add(i, 1) == ORBX_OK);
        full.commit_add(i);
    }
    CHECK(full.size == kKfdbMaxMembers && full.hi == kKfdbMaxMembers && full.check_add(kKfdbMaxMembers, 1) == ORBX_ERR_ARG);

    CHECK(kfdb_sort_len(0) == 2 && kfdb_sort_len(1) == 2 && kfdb_sort_len(2) == 2 && kfdb_sort_len(3) == 4);
    CHECK(kfdb_sort_len(64) == 64 && kfdb_sort_len(65) == 128 && kfdb_sort_len(8192) == 8192);
    std::puts("kfdb host ok");
    return 0;
}
