// The host side of the essential-graph optimisation (orbx_essgraph.hip), free
// of HIP and of the context so that it compiles and is tested on its own
// (tests/essgraph_check.cpp): the checks of the graph's ids and edges, and the
// symbolic part of the block Cholesky of H + lambda I.
//
// The free vertices are the keyframes other than the fixed one that have an
// edge, in id order (g2o: sortVectorContainers, buildIndexMapping).  Storage
// is the envelope (skyline) by block row: first[r] is the smallest free index
// row r is connected to (or r), row r stores the 7 x 7 blocks first[r]..r, and
// a Cholesky factor fills only inside the envelope, so no ordering heuristic
// and no elimination tree is needed: the essential graph is narrow in id
// order, with a few long rows where loop edges land.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "orbx.h"

namespace orbx {

struct EssPlan {
    int n_free = 0, max_row_blocks = 0;
    long long n_blocks = 0;
    std::vector<int32_t> free_of_kf;   // n_kf: the free index of a keyframe, -1 outside the system
    std::vector<int32_t> kf_of_free;   // n_free
    std::vector<int32_t> first;        // n_free
    std::vector<int64_t> row_off;      // n_free + 1, in blocks
    std::vector<int64_t> col_off;      // n_free + 1: per column c, the rows r > c whose envelope holds c
    std::vector<int32_t> col_rows;     // n_blocks - n_free, ascending per column
    std::vector<int32_t> inc_off;      // n_free + 1: per free vertex, its edges in g2o's order
    std::vector<int32_t> inc_edge;     // edge << 1 | side (0: the vertex is i, 1: it is j)
};

// ORBX_ERR_ARG for duplicate ids, an edge index outside [0, n_kf), i == j or a
// kind other than 0 / 1, a fixed index outside [-1, n_kf).
inline int essgraph_check(int n_kf, const int64_t* ids, int fixed, int n_edges, const orbx_essgraph_edge* edges)
{
    if (n_kf < 0 || n_edges < 0 || (n_kf > 0 && !ids) || (n_edges > 0 && !edges)) return ORBX_ERR_ARG;
    if (fixed < -1 || fixed >= n_kf) return ORBX_ERR_ARG;
    std::vector<int64_t> sorted(ids, ids + n_kf);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return ORBX_ERR_ARG;
    for (int e = 0; e < n_edges; e++) {
        const orbx_essgraph_edge& E = edges[e];
        if (E.i < 0 || E.i >= n_kf || E.j < 0 || E.j >= n_kf || E.i == E.j || E.kind > 1) return ORBX_ERR_ARG;
    }
    return ORBX_OK;
}

// The free vertices of a checked graph in id order and each one's first column.
inline void essgraph_rows(int n_kf, const int64_t* ids, int fixed, int n_edges, const orbx_essgraph_edge* edges,
                          EssPlan& P)
{
    std::vector<uint8_t> has_edge(n_kf, 0);
    for (int e = 0; e < n_edges; e++) has_edge[edges[e].i] = has_edge[edges[e].j] = 1;
    std::vector<int32_t> by_id(n_kf);
    std::iota(by_id.begin(), by_id.end(), 0);
    std::sort(by_id.begin(), by_id.end(), [&](int a, int b) { return ids[a] < ids[b]; });
    P.free_of_kf.assign(n_kf, -1);
    for (int k : by_id)
        if (k != fixed && has_edge[k]) {
            P.free_of_kf[k] = (int32_t)P.kf_of_free.size();
            P.kf_of_free.push_back(k);
        }
    const int n = P.n_free = (int)P.kf_of_free.size();
    P.first.resize(n);
    std::iota(P.first.begin(), P.first.end(), 0);
    for (int e = 0; e < n_edges; e++) {
        const int a = P.free_of_kf[edges[e].i], b = P.free_of_kf[edges[e].j];
        if (a >= 0 && b >= 0) P.first[std::max(a, b)] = std::min(P.first[std::max(a, b)], std::min(a, b));
    }
    P.n_blocks = 0;
    for (int r = 0; r < n; r++) P.n_blocks += r - P.first[r] + 1;
}

// n_blocks of a checked graph without the lists (the cap is tested before they are built).
inline long long essgraph_blocks(int n_kf, const int64_t* ids, int fixed, int n_edges, const orbx_essgraph_edge* edges)
{
    EssPlan P;
    essgraph_rows(n_kf, ids, fixed, n_edges, edges, P);
    return P.n_blocks;
}

// The plan of a checked graph.
inline EssPlan essgraph_plan(int n_kf, const int64_t* ids, int fixed, int n_edges, const orbx_essgraph_edge* edges)
{
    EssPlan P;
    essgraph_rows(n_kf, ids, fixed, n_edges, edges, P);
    const int n = P.n_free;
    P.inc_off.assign(n + 1, 0);
    for (int e = 0; e < n_edges; e++) {
        const int a = P.free_of_kf[edges[e].i], b = P.free_of_kf[edges[e].j];
        if (a >= 0) P.inc_off[a + 1]++;
        if (b >= 0) P.inc_off[b + 1]++;
    }
    for (int r = 0; r < n; r++) P.inc_off[r + 1] += P.inc_off[r];
    P.inc_edge.resize(P.inc_off[n]);
    {
        std::vector<int32_t> at(P.inc_off.begin(), P.inc_off.end() - 1);
        for (int e = 0; e < n_edges; e++) {
            const int a = P.free_of_kf[edges[e].i], b = P.free_of_kf[edges[e].j];
            if (a >= 0) P.inc_edge[at[a]++] = e << 1;
            if (b >= 0) P.inc_edge[at[b]++] = e << 1 | 1;
        }
    }
    P.row_off.assign(n + 1, 0);
    P.col_off.assign(n + 1, 0);
    for (int r = 0; r < n; r++) {
        const int len = r - P.first[r] + 1;
        P.row_off[r + 1] = P.row_off[r] + len;
        P.max_row_blocks = std::max(P.max_row_blocks, len);
        for (int c = P.first[r]; c < r; c++) P.col_off[c + 1]++;
    }
    for (int c = 0; c < n; c++) P.col_off[c + 1] += P.col_off[c];
    P.col_rows.resize(P.col_off[n]);
    {
        std::vector<int64_t> at(P.col_off.begin(), P.col_off.end() - 1);
        for (int r = 0; r < n; r++)
            for (int c = P.first[r]; c < r; c++) P.col_rows[at[c]++] = r;
    }
    return P;
}

}  // namespace orbx
