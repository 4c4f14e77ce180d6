// Host-side bookkeeping of the device keyframe database (orbx_kfdb.hip): which
// ids are members, the add counter that orders the inverted-file lists, and
// the argument checks of every entry point.  Standard headers only (plus the
// error codes of orbx.h, itself standard C), so that it compiles and is
// checked on its own (tests/kfdb_host_check.cpp).
//
// The reference keeps a std::list<KeyFrame*> per word (src/KeyFrameDatabase.cc:
// 39-66): add() appends, erase() removes and keeps the others' relative order.
// A list's order is therefore the order of the members' add() calls, and one
// counter per database that grows with every add reproduces it: a member that
// is erased and added again goes to the back, as it does in the lists.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/orbx.h"

namespace orbx {

constexpr int kKfdbMaxMembers = ORBX_KFDB_MAX_MEMBERS;
constexpr int kKfdbMaxWords = ORBX_KFDB_MAX_WORDS;
constexpr int kKfdbNeigh = ORBX_KFDB_NEIGHBOURS;

struct KfdbTable {
    int capacity = 0, max_words = 0;
    int size = 0;        // members
    int hi = 0;          // one past the largest id ever used since clear()
    uint32_t next_seq = 0;
    std::vector<uint8_t> member;   // [capacity]

    static int check_create(int capacity, int max_words)
    {
        if (capacity < 1 || max_words < 1) return ORBX_ERR_ARG;
        if (capacity > kKfdbMaxMembers || max_words > kKfdbMaxWords) return ORBX_ERR_UNSUPPORTED;
        return ORBX_OK;
    }
    int create(int cap, int words)
    {
        const int r = check_create(cap, words);
        if (r != ORBX_OK) return r;
        capacity = cap;
        max_words = words;
        member.assign((size_t)cap, 0);
        clear();
        return ORBX_OK;
    }
    void clear()
    {
        member.assign(member.size(), 0);
        size = 0;
        hi = 0;
        next_seq = 0;
    }
    bool in_range(int id) const { return id >= 0 && id < capacity; }
    bool is_member(int id) const { return in_range(id) && member[(size_t)id]; }

    // words strictly ascending (a std::map's iteration), values finite
    static bool bow_ok(int n, const uint32_t* words, const double* values)
    {
        if (n < 0 || (n > 0 && (!words || !values))) return false;
        for (int i = 0; i < n; i++) {
            if (i > 0 && words[i] <= words[i - 1]) return false;
            if (!std::isfinite(values[i])) return false;
        }
        return true;
    }
    // the id may be added (n_words < 0: the count is known on the device only)
    int check_add(int id, int n_words) const
    {
        if (!in_range(id) || member[(size_t)id]) return ORBX_ERR_ARG;
        if (n_words > max_words) return ORBX_ERR_CAPACITY;
        if (next_seq == UINT32_MAX) return ORBX_ERR_UNSUPPORTED;   // 2^32 - 1 adds since clear()
        return ORBX_OK;
    }
    // after check_add: the member's sequence number
    uint32_t commit_add(int id)
    {
        member[(size_t)id] = 1;
        size++;
        if (id + 1 > hi) hi = id + 1;
        return next_seq++;
    }
    int check_erase(int id) const { return is_member(id) ? ORBX_OK : ORBX_ERR_ARG; }
    void commit_erase(int id)
    {
        member[(size_t)id] = 0;
        size--;
    }
    // every id of a list names a possible member (a non-member is skipped by
    // the query; an id outside [0, capacity) is the caller's mistake)
    int check_ids(int n, const int32_t* ids) const
    {
        if (n < 0 || (n > 0 && !ids)) return ORBX_ERR_ARG;
        for (int i = 0; i < n; i++)
            if (!in_range(ids[i])) return ORBX_ERR_ARG;
        return ORBX_OK;
    }
    int check_members(int n, const int32_t* ids) const
    {
        if (n < 0 || (n > 0 && !ids)) return ORBX_ERR_ARG;
        for (int i = 0; i < n; i++)
            if (!is_member(ids[i])) return ORBX_ERR_ARG;
        return ORBX_OK;
    }
};

// The smallest power of two >= n (n >= 1), at least 2: the length the block
// sort of the select kernel runs on.
inline int kfdb_sort_len(int n)
{
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace orbx
