// Host-side bookkeeping of the device covisibility map (orbx_covis.hip): which
// ids are members or erased, the order of the keyframes' keys, a shadow of
// every member's map-point row with the observers of every point, and the
// argument checks of every edit.  Standard headers only (plus the error codes
// of orbx.h, itself standard C), so that it compiles and is checked on its own
// (tests/covis_host_check.cpp).
//
// The reference orders its std::map<KeyFrame*, ...> and its sorted
// pair<int, KeyFrame*> by pointer value.  The caller hands that value over as a
// 64-bit key per keyframe; all the device needs of it is the order, so the
// table keeps every key ever added sorted and gives each keyframe its rank.
// A rank fits 13 bits, which lets the kernels compare (weight, key) as one
// 32-bit word.  An add that lands between two keys shifts the ranks above it:
// the caller uploads ranks() again after every add.
//
// A point stands at most once in a row (MapPoint::mObservations holds one
// index per keyframe).  obs[p] lists the cells (keyframe, index) that hold p,
// which answers "is p in this row" for the check and names the cells that
// erase_points clears.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/orbx.h"

namespace orbx {

constexpr int kCovisMaxKeyframes = ORBX_COVIS_MAX_KEYFRAMES;
constexpr int kCovisMaxKeypoints = ORBX_COVIS_MAX_KEYPOINTS;
constexpr int kCovisMaxPoints = ORBX_COVIS_MAX_POINTS;
constexpr int kCovisRankBits = 13;   // 2^13 = kCovisMaxKeyframes
static_assert((1 << kCovisRankBits) == kCovisMaxKeyframes, "a rank fits kCovisRankBits");

struct CovisTable {
    enum : uint8_t { kFree = 0, kMember = 1, kErased = 2 };
    int kf_capacity = 0, mp_capacity = 0, max_keypoints = 0;
    int size = 0;   // members
    int hi = 0;     // one past the largest id ever added since clear()
    std::vector<uint8_t> state;                             // [kf_capacity]
    std::vector<std::pair<uint64_t, int32_t>> sorted_keys;  // every key ever added, ascending, with its id
    std::vector<int32_t> rank;                              // [kf_capacity] id -> place in sorted_keys, -1
    std::vector<int32_t> by_rank;                           // [kf_capacity] its inverse, -1 padded
    std::vector<std::vector<int32_t>> rows;                 // [kf_capacity] a member's row
    std::vector<uint8_t> erased;                            // [mp_capacity]
    std::vector<std::vector<uint32_t>> obs;                 // [mp_capacity] cells id << 16 | index

    static uint32_t cell(int id, int idx) { return (uint32_t)id << 16 | (uint32_t)idx; }
    static int cell_kf(uint32_t c) { return (int)(c >> 16); }
    static int cell_idx(uint32_t c) { return (int)(c & 0xFFFFu); }

    static int check_create(int kf_cap, int mp_cap, int max_kp)
    {
        if (kf_cap < 1 || mp_cap < 1 || max_kp < 1) return ORBX_ERR_ARG;
        if (kf_cap > kCovisMaxKeyframes || max_kp > kCovisMaxKeypoints || mp_cap > kCovisMaxPoints)
            return ORBX_ERR_UNSUPPORTED;
        return ORBX_OK;
    }
    int create(int kf_cap, int mp_cap, int max_kp)
    {
        const int r = check_create(kf_cap, mp_cap, max_kp);
        if (r != ORBX_OK) return r;
        kf_capacity = kf_cap;
        mp_capacity = mp_cap;
        max_keypoints = max_kp;
        clear();
        return ORBX_OK;
    }
    void clear()
    {
        state.assign((size_t)kf_capacity, kFree);
        sorted_keys.clear();
        rank.assign((size_t)kf_capacity, -1);
        by_rank.assign((size_t)kf_capacity, -1);
        rows.assign((size_t)kf_capacity, std::vector<int32_t>());
        erased.assign((size_t)mp_capacity, 0);
        obs.assign((size_t)mp_capacity, std::vector<uint32_t>());
        octaves_set.assign((size_t)kf_capacity, 0);
        size = 0;
        hi = 0;
    }
    bool kf_in_range(int id) const { return id >= 0 && id < kf_capacity; }
    bool is_member(int id) const { return kf_in_range(id) && state[(size_t)id] == kMember; }
    bool point_ok(int p) const { return p >= -1 && p < mp_capacity; }   // -1: no point
    bool key_used(uint64_t key) const
    {
        auto it = std::lower_bound(sorted_keys.begin(), sorted_keys.end(), std::make_pair(key, INT32_MIN));
        return it != sorted_keys.end() && it->first == key;
    }
    bool in_row(int id, int p) const
    {
        for (uint32_t c : obs[(size_t)p])
            if (cell_kf(c) == id) return true;
        return false;
    }

    // entries -1 or a point id, no point twice
    bool row_ok(int n, const int32_t* mp) const
    {
        if (n < 0 || n > max_keypoints || (n > 0 && !mp)) return false;
        std::vector<int32_t> s;
        s.reserve((size_t)n);
        for (int i = 0; i < n; i++) {
            if (!point_ok(mp[i])) return false;
            if (mp[i] >= 0) s.push_back(mp[i]);
        }
        std::sort(s.begin(), s.end());
        return std::adjacent_find(s.begin(), s.end()) == s.end();
    }
    int check_add(int id, uint64_t key, int n, const int32_t* mp) const
    {
        if (!kf_in_range(id) || state[(size_t)id] != kFree) return ORBX_ERR_ARG;   // in use, or erased: never reused
        if (key_used(key) || !row_ok(n, mp)) return ORBX_ERR_ARG;
        return ORBX_OK;
    }
    // after check_add; the ranks of the keys above the new one move up
    void commit_add(int id, uint64_t key, int n, const int32_t* mp)
    {
        const auto entry = std::make_pair(key, (int32_t)id);
        const auto it = sorted_keys.insert(std::lower_bound(sorted_keys.begin(), sorted_keys.end(), entry), entry);
        for (size_t r = (size_t)(it - sorted_keys.begin()); r < sorted_keys.size(); r++) {
            rank[(size_t)sorted_keys[r].second] = (int32_t)r;
            by_rank[r] = sorted_keys[r].second;
        }
        std::vector<int32_t>& row = rows[(size_t)id];
        row.assign(mp, mp + n);
        for (int i = 0; i < n; i++)
            if (row[(size_t)i] >= 0) obs[(size_t)row[(size_t)i]].push_back(cell(id, i));
        state[(size_t)id] = kMember;
        size++;
        if (id + 1 > hi) hi = id + 1;
    }

    void unobserve(int p, int id)
    {
        std::vector<uint32_t>& o = obs[(size_t)p];
        for (size_t k = 0; k < o.size(); k++)
            if (cell_kf(o[k]) == id) {
                o[k] = o.back();
                o.pop_back();
                return;
            }
    }
    // one cell of a member's row; false when p already stands elsewhere in it
    bool write_cell(int id, int idx, int p)
    {
        int32_t& slot = rows[(size_t)id][(size_t)idx];
        if (slot == p) return true;
        if (p >= 0 && in_row(id, p)) return false;
        if (slot >= 0) unobserve(slot, id);
        slot = p;
        if (p >= 0) obs[(size_t)p].push_back(cell(id, idx));
        return true;
    }
    // The edits in order, all or none: an index outside the row, a point out of
    // range or a point that would stand twice undoes the edits before it.
    int set_matches(int id, int n_edits, const int32_t* idx, const int32_t* mp)
    {
        if (!is_member(id) || n_edits < 0 || (n_edits > 0 && (!idx || !mp))) return ORBX_ERR_ARG;
        const int n = (int)rows[(size_t)id].size();
        std::vector<std::pair<int32_t, int32_t>> undo;
        undo.reserve((size_t)n_edits);
        for (int k = 0; k < n_edits; k++) {
            const bool ok = idx[k] >= 0 && idx[k] < n && point_ok(mp[k]);
            const int32_t old = ok ? rows[(size_t)id][(size_t)idx[k]] : -1;
            if (!ok || !write_cell(id, idx[k], mp[k])) {
                // back to front: the states the edits went through, each of them valid
                for (size_t u = undo.size(); u-- > 0;) write_cell(id, undo[u].first, undo[u].second);
                return ORBX_ERR_ARG;
            }
            undo.emplace_back(idx[k], old);
        }
        return ORBX_OK;
    }

    int check_points(int n, const int32_t* ids) const
    {
        if (n < 0 || (n > 0 && !ids)) return ORBX_ERR_ARG;
        for (int i = 0; i < n; i++)
            if (ids[i] < 0 || ids[i] >= mp_capacity) return ORBX_ERR_ARG;
        return ORBX_OK;
    }
    // after check_points: marks the points and clears them from every row;
    // `cells` receives the cleared cells (for the device's copy of the rows)
    void erase_points(int n, const int32_t* ids, std::vector<uint32_t>& cells)
    {
        for (int i = 0; i < n; i++) {
            const size_t p = (size_t)ids[i];
            erased[p] = 1;
            for (uint32_t c : obs[p]) {
                rows[(size_t)cell_kf(c)][(size_t)cell_idx(c)] = -1;
                cells.push_back(c);
            }
            obs[p].clear();
        }
    }

    int check_erase_keyframe(int id) const { return is_member(id) ? ORBX_OK : ORBX_ERR_ARG; }
    // the id keeps its key and rank: a stale entry of another row still sorts by it
    void commit_erase_keyframe(int id)
    {
        std::vector<int32_t>& row = rows[(size_t)id];
        for (int32_t p : row)
            if (p >= 0) unobserve(p, id);
        std::vector<int32_t>().swap(row);
        state[(size_t)id] = kErased;
        size--;
    }
    int check_members(int n, const int32_t* ids) const
    {
        if (n < 0 || (n > 0 && !ids)) return ORBX_ERR_ARG;
        for (int i = 0; i < n; i++)
            if (!is_member(ids[i])) return ORBX_ERR_ARG;
        return ORBX_OK;
    }
    // a frame's mvpMapPoints: -1 or a point id (it may hold a point twice)
    bool frame_ok(int n, const int32_t* mp) const
    {
        if (n < 0 || n > max_keypoints || (n > 0 && !mp)) return false;
        for (int i = 0; i < n; i++)
            if (!point_ok(mp[i])) return false;
        return true;
    }

    // ---- the culling walks (orbx_covis_set_octaves, _cull_keyframes, _cull_points) ----
    // The octaves themselves live in HBM alone; the shadow knows who has them.
    std::vector<uint8_t> octaves_set;   // [kf_capacity]

    int check_octaves(int id, int n, const uint8_t* octave) const
    {
        if (!is_member(id) || n != (int)rows[(size_t)id].size() || (n > 0 && !octave)) return ORBX_ERR_ARG;
        return ORBX_OK;
    }
    void commit_octaves(int id) { octaves_set[(size_t)id] = 1; }
    bool has_octaves(int id) const { return octaves_set[(size_t)id] != 0; }
    bool every_member_has_octaves() const
    {
        for (int id = 0; id < hi; id++)
            if (state[(size_t)id] == kMember && !has_octaves(id)) return false;
        return true;
    }
    // the cells of all member rows: what bounds the observer cells and the bad points of one cull call
    size_t member_cells() const
    {
        size_t s = 0;
        for (int id = 0; id < hi; id++)
            if (state[(size_t)id] == kMember) s += rows[(size_t)id].size();
        return s;
    }
    bool ids_in_range(int n, const int32_t* ids) const
    {
        if (n < 0 || (n > 0 && !ids)) return false;
        for (int k = 0; k < n; k++)
            if (!kf_in_range(ids[k])) return false;
        return true;
    }
    // The arguments of orbx_covis_cull_keyframes, before any device work.
    int check_cull(const orbx_covis_cull_args* q) const
    {
        if (!q || q->max_culls < 0 || q->cand_cap < 0 || q->bad_cap < 0 || !ids_in_range(q->n_keep, q->keep))
            return ORBX_ERR_ARG;
        if ((q->cand_cap > 0 && (!q->cand || !q->n_mps || !q->n_redundant || !q->decision)) ||
            (q->bad_cap > 0 && !q->bad_points))
            return ORBX_ERR_ARG;
        if (q->cur == -1) {
            if (q->n_cand > kf_capacity || !ids_in_range(q->n_cand, q->cand)) return ORBX_ERR_ARG;
        } else if (!is_member(q->cur)) {
            return ORBX_ERR_ARG;
        }
        if (!every_member_has_octaves()) return ORBX_ERR_ARG;
        if (q->cur == -1 && q->n_cand > q->cand_cap) return ORBX_ERR_CAPACITY;
        return ORBX_OK;
    }
    // What one cull call read back: all or none.  A count above its capacity
    // changes nothing (the device left its state alone too); otherwise every
    // culled keyframe goes as commit_erase_keyframe takes it and every bad
    // point as erase_points takes it.  The end state does not depend on the
    // order of the two kinds: a row that went no longer holds the point, a
    // point that went no longer stands in the row.
    int apply_cull(int n_cand, int cand_cap, int n_done, const int32_t* cand, const int32_t* decision, int n_bad,
                   int bad_cap, const int32_t* bad)
    {
        if (n_cand > cand_cap || n_bad > bad_cap) return ORBX_ERR_CAPACITY;
        if (n_done < 0 || n_done > n_cand || n_bad < 0 || check_points(n_bad, bad) != ORBX_OK) return ORBX_ERR_ARG;
        for (int k = 0; k < n_done; k++)
            if (decision[k] == 1 && !is_member(cand[k])) return ORBX_ERR_ARG;
        for (int k = 0; k < n_done; k++)
            if (decision[k] == 1) commit_erase_keyframe(cand[k]);
        std::vector<uint32_t> cells;
        erase_points(n_bad, bad, cells);
        return ORBX_OK;
    }

    // The arguments of orbx_covis_cull_points.
    int check_cull_points(int cur_kf, int n, const int32_t* ids, const int32_t* found, const int32_t* visible,
                          const int32_t* first_kf, const int32_t* action) const
    {
        if (cur_kf < 0 || check_points(n, ids) != ORBX_OK || (n > 0 && (!found || !visible || !first_kf || !action)))
            return ORBX_ERR_ARG;
        for (int k = 0; k < n; k++)
            if (found[k] < 0 || visible[k] < 0 || first_kf[k] < 0 || first_kf[k] > cur_kf) return ORBX_ERR_ARG;
        std::vector<int32_t> s(ids, ids + n);
        std::sort(s.begin(), s.end());
        return std::adjacent_find(s.begin(), s.end()) == s.end() ? ORBX_OK : ORBX_ERR_ARG;
    }
    // the points of actions 2 and 3 go
    void apply_cull_points(int n, const int32_t* ids, const int32_t* action)
    {
        std::vector<int32_t> gone;
        for (int k = 0; k < n; k++)
            if (action[k] == 2 || action[k] == 3) gone.push_back(ids[k]);
        std::vector<uint32_t> cells;
        erase_points((int)gone.size(), gone.data(), cells);
    }
};

// The smallest power of two >= n, at least 2: the length the block sort of
// the list kernel runs on.
inline int covis_sort_len(int n)
{
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace orbx
