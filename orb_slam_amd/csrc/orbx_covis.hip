// The covisibility graph on MI355X: the keyframe -> map-point table and the
// connection weights in HBM, with KeyFrame::UpdateConnections
// (src/KeyFrame.cc:332-421), the covisibility reads (:162-211) and
// Tracking::UpdateReferenceKeyFrames / UpdateReferencePoints
// (src/Tracking.cc:764-865) as kernels over them.  Integer arithmetic only.
//
// The reference walks MapPoint::mObservations (a std::map<KeyFrame*, size_t>
// per point) to count, for a set of points, how often each keyframe sees one
// of them.  Here the set is stamped into a per-point mark array (the
// occurrence count of every point of the frame, or of row i) and every member
// row is scanned once:
//
//   k_covis_mark     the occurrence counts of a frame's (or a row's) points;
//                    integer atomic adds, so the order of arrival is nothing.
//   k_covis_count    one wavefront per member row: the sum of its entries'
//                    marks is the keyframe's vote (counter[j]).
//   k_covis_select   one workgroup: the voters in key order, pKFmax; it also
//                    zeroes the marks the frame left.
//   k_covis_top      one workgroup per voter (at most 80): the first 10 of
//                    its ordered list, by ten rounds of a (weight, key) maximum.
//   k_covis_pass     the neighbour pass, sequential by nature: one thread.
//   k_covis_first / _tally / _emit
//                    mvpLocalMapPoints: the minimum (list position, index) per
//                    point, the winners per keyframe, the ordered emission.
//   k_covis_connect  one workgroup: the W and flag updates of one
//                    UpdateConnections; they take effect in ids order because
//                    the launches of one call follow each other on the stream.
//   k_covis_list     one workgroup: an ordered list (or a row in key order),
//                    sorted in LDS.
//   k_cull_* / k_cullp_*
//                    LocalMapping's KeyFrameCulling and MapPointCulling, with
//                    the keypoint octaves beside the rows: described where
//                    they stand, below.
//
// Order.  The host keeps every key ever added sorted and uploads each
// keyframe's rank (orbx_covis_host.h), so (weight, key) compares as the word
// weight << 13 | rank, and "ascending key" is a scatter by rank.
#include <climits>
#include <new>
#include <vector>

#include "orbx_covis_host.h"
#include "orbx_device.h"
#include "orbx_internal.h"
#include "orbx_stage.h"

namespace orbx {

constexpr int kCovisThreads = 256;           // mark, count, top, first, tally, emit
constexpr int kCovisWaves = kCovisThreads / 64;
constexpr int kCovisBlock = 1024;            // select, connect, list
constexpr int kCovisLocalLimit = 80;         // `if(mvpLocalKeyFrames.size()>80) break;`
constexpr int kCovisBest = 10;               // GetBestCovisibilityKeyFrames(10)
constexpr int kRankMask = (1 << kCovisRankBits) - 1;
constexpr int kCovisHeader = 8;              // ints: n_local_kf, n_voters, ref_kf, n_local_mp

struct CovisDev {
    // the table
    int32_t* rows;      // kf_capacity x max_keypoints
    int32_t* row_n;     // a member's row length; -1: not a member
    int32_t* rank;      // the place of the keyframe's key among all keys; -1: never added
    int32_t* by_rank;
    uint8_t* erased;    // per point
    // the connection state
    uint16_t* W;        // kf_capacity x w_stride; 0: no entry
    int32_t* filt;
    int32_t* th;
    // the running call
    int32_t* mark;      // per point: occurrences in the frame / row; zero between calls
    uint32_t* first;    // per point: min (list position << 16 | index); ~0 between calls
    int32_t* votes;     // per keyframe
    uint8_t* incl;      // per keyframe: in the local list
    int32_t* top;       // kCovisLocalLimit x kCovisBest
    int32_t* cnt;       // per list position: the points that stand there first
    int32_t* lkf;       // mvpLocalKeyFrames
    int32_t* lmp;       // mvpLocalMapPoints
    int32_t* hdr;       // kCovisHeader
    int32_t* res;       // update_connections: 2 per id; connections: 1 + 2 cap
    int32_t* edit;      // an uploaded frame, or erase_points' cells and ids
    uint8_t* ferased;   // per frame entry
    uint8_t* oct;       // kf_capacity x max_keypoints: mvKeysUn[i].octave, beside rows
};

__device__ inline bool covis_point(int p, int M) { return p >= 0 && p < M; }

// The occurrence count of every point of src[0, n) that is not erased.
__global__ __launch_bounds__(kCovisThreads) void k_covis_mark(CovisDev d, const int32_t* src, int n, int M,
                                                              uint8_t* ferased)
{
    const int i = blockIdx.x * kCovisThreads + threadIdx.x;
    if (i >= n) return;
    const int p = src[i];
    bool e = false;
    if (covis_point(p, M)) {
        if (d.erased[p]) e = true;
        else atomicAdd(&d.mark[p], 1);
    }
    if (ferased) ferased[i] = e ? 1 : 0;
}

// Rows [0, hi), a wavefront each: votes[j] = the marks of row j's entries
// (0 for j == skip and for an id that is no member).
__global__ __launch_bounds__(kCovisThreads) void k_covis_count(CovisDev d, int hi, int P, int M, int skip)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * kCovisWaves + (threadIdx.x >> 6);
    if (j >= hi) return;   // the whole wavefront
    const int n = j == skip ? 0 : min(d.row_n[j], P);
    const int32_t* row = d.rows + (size_t)j * P;
    int s = 0;
    for (int i = lane; i < n; i += 64) {
        const int p = row[i];
        if (covis_point(p, M)) s += d.mark[p];
    }
    s = wave_sum(s);
    if (lane == 0) d.votes[j] = s;
}

// After k_covis_count of a frame.  Dynamic LDS: nr ints, a slot per rank.
__global__ __launch_bounds__(kCovisBlock) void k_covis_select(CovisDev d, int hi, int nr, const int32_t* frame, int nf,
                                                              int M)
{
    extern __shared__ int32_t s_slot[];
    __shared__ BlockScratchN<kCovisBlock / 64> bs;
    const int tid = threadIdx.x;
    for (int i = tid; i < nf; i += kCovisBlock) {   // the frame's marks are used up
        const int p = frame[i];
        if (covis_point(p, M)) d.mark[p] = 0;
    }
    for (int r = tid; r < nr; r += kCovisBlock) s_slot[r] = -1;
    __syncthreads();
    int best = 0;   // votes << 13 | (mask - rank): the first strict maximum in ascending key order
    for (int j = tid; j < hi; j += kCovisBlock) {
        const int v = d.row_n[j] >= 0 ? d.votes[j] : 0;
        const int r = d.rank[j];
        const bool voter = v > 0 && r >= 0 && r < nr;
        d.incl[j] = voter ? 1 : 0;
        if (voter) {
            s_slot[r] = j;
            best = max(best, v << kCovisRankBits | (kRankMask - r));
        }
    }
    best = block_max(best, bs, 0);   // a barrier: the slots are written
    const int per = (nr + kCovisBlock - 1) / kCovisBlock;
    const int r0 = min(tid * per, nr), r1 = min(r0 + per, nr);
    int mine = 0;
    for (int r = r0; r < r1; r++) mine += s_slot[r] >= 0;
    int nv = 0;
    int o = block_exclusive_scan(mine, &nv, bs, 1);
    for (int r = r0; r < r1; r++)
        if (s_slot[r] >= 0) d.lkf[o++] = s_slot[r];
    if (tid == 0) {
        d.hdr[0] = nv;
        d.hdr[1] = nv;
        d.hdr[2] = best ? d.by_rank[kRankMask - (best & kRankMask)] : -1;
        d.hdr[3] = 0;
    }
}

// The first kCovisBest entries of the ordered list of voter blockIdx.x, -1
// padded.  Nothing to do when the neighbour pass will not run.
__global__ __launch_bounds__(kCovisThreads) void k_covis_top(CovisDev d, int hi, int Ws)
{
    __shared__ BlockScratchN<kCovisWaves> bs;
    const int nv = d.hdr[1];
    const int l = blockIdx.x, tid = threadIdx.x;
    if (nv > kCovisLocalLimit || l >= nv) return;
    const int v = d.lkf[l];
    const uint16_t* w = d.W + (size_t)v * Ws;
    const bool filtered = d.filt[v] != 0;
    const int th = filtered ? d.th[v] : 1;
    int32_t* out = d.top + l * kCovisBest;
    int prev = INT_MAX, got = 0;
    for (; got < kCovisBest; got++) {   // the largest (weight, key) below the one before
        int best = 0;
        for (int j = tid; j < hi; j += kCovisThreads) {
            const int x = w[j];
            if (x < th) continue;
            const int r = d.rank[j];
            const int pk = x << kCovisRankBits | r;
            if (r >= 0 && pk < prev) best = max(best, pk);
        }
        best = block_max(best, bs, got & 1);
        if (best == 0) break;
        if (tid == 0) out[got] = d.by_rank[best & kRankMask];
        prev = best;
    }
    if (got == 0 && filtered) {   // none reaches th: the largest weight, the smallest key among equals
        int best = 0;
        for (int j = tid; j < hi; j += kCovisThreads) {
            const int x = w[j], r = d.rank[j];
            if (x > 0 && r >= 0) best = max(best, x << kCovisRankBits | (kRankMask - r));
        }
        best = block_max(best, bs, 1);   // the loop above left after its use of buffer 0
        if (best) {
            if (tid == 0) out[0] = d.by_rank[kRankMask - (best & kRankMask)];
            got = 1;
        }
    }
    for (int k = got + tid; k < kCovisBest; k += kCovisThreads) out[k] = -1;
}

// src/Tracking.cc:838-862, one thread.
__global__ void k_covis_pass(CovisDev d, int hi)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int nv = d.hdr[1];
    int size = nv;
    const int visit = nv > kCovisLocalLimit ? 0 : nv;
    for (int l = 0; l < visit; l++) {
        if (size > kCovisLocalLimit) break;
        for (int t = 0; t < kCovisBest; t++) {
            const int j = d.top[l * kCovisBest + t];
            if (j < 0) break;                               // the list has ended
            if (j >= hi || d.row_n[j] < 0) continue;        // isBad(): the place is taken, the entry skipped
            if (!d.incl[j]) {
                d.lkf[size++] = j;
                d.incl[j] = 1;
                break;
            }
        }
    }
    d.hdr[0] = size;
}

// Workgroup l: row of the l-th local keyframe.
__global__ __launch_bounds__(kCovisThreads) void k_covis_first(CovisDev d, int P, int M)
{
    const int l = blockIdx.x;
    if (l >= d.hdr[0]) return;
    const int kf = d.lkf[l], n = min(d.row_n[kf], P);
    const int32_t* row = d.rows + (size_t)kf * P;
    for (int i = threadIdx.x; i < n; i += kCovisThreads) {
        const int p = row[i];
        if (covis_point(p, M) && !d.erased[p]) atomicMin(&d.first[p], (uint32_t)l << 16 | (uint32_t)i);
    }
}

__device__ inline bool covis_stands_first(const CovisDev& d, int p, int M, int l, int i)
{
    // written by atomics, which act in L2: read it there
    return covis_point(p, M) && !d.erased[p] &&
           __hip_atomic_load(&d.first[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ((uint32_t)l << 16 | (uint32_t)i);
}

__global__ __launch_bounds__(kCovisThreads) void k_covis_tally(CovisDev d, int P, int M)
{
    __shared__ BlockScratchN<kCovisWaves> bs;
    const int l = blockIdx.x;
    if (l >= d.hdr[0]) return;
    const int kf = d.lkf[l], n = min(d.row_n[kf], P);
    const int32_t* row = d.rows + (size_t)kf * P;
    int c = 0;
    for (int i = threadIdx.x; i < n; i += kCovisThreads) c += covis_stands_first(d, row[i], M, l, i);
    c = block_sum(c, bs, 0);
    if (threadIdx.x == 0) d.cnt[l] = c;
}

// The points of row l that stand there first, in index order, behind those of
// the rows before; their `first` entries go back to ~0.
__global__ __launch_bounds__(kCovisThreads) void k_covis_emit(CovisDev d, int P, int M)
{
    __shared__ BlockScratchN<kCovisWaves> bs;
    const int l = blockIdx.x, nl = d.hdr[0];
    if (l >= nl) return;
    int before = 0;
    for (int k = threadIdx.x; k < l; k += kCovisThreads) before += d.cnt[k];
    int base = block_sum(before, bs, 0);
    const int kf = d.lkf[l], n = min(d.row_n[kf], P);
    const int32_t* row = d.rows + (size_t)kf * P;
    int buf = 1;
    for (int i0 = 0; i0 < n; i0 += kCovisThreads, buf ^= 1) {
        const int i = i0 + threadIdx.x;
        const int p = i < n ? row[i] : -1;
        const bool win = i < n && covis_stands_first(d, p, M, l, i);
        int total = 0;
        const int o = block_exclusive_scan(win ? 1 : 0, &total, bs, buf);
        if (win) {
            d.lmp[base + o] = p;
            d.first[p] = 0xFFFFFFFFu;   // no other cell equals it, before or after this store
        }
        base += total;
    }
    if (l == nl - 1 && threadIdx.x == 0) d.hdr[3] = base;
}

// One UpdateConnections of member i after k_covis_mark of its row and
// k_covis_count with skip = i.  res: updated, front.
__global__ __launch_bounds__(kCovisBlock) void k_covis_connect(CovisDev d, int hi, int Ws, int P, int M, int i, int th,
                                                               int32_t* res)
{
    __shared__ BlockScratchN<kCovisBlock / 64> bs;
    const int tid = threadIdx.x;
    const int n = min(d.row_n[i], P);
    const int32_t* row = d.rows + (size_t)i * P;
    for (int k = tid; k < n; k += kCovisBlock) {   // the row's marks are used up
        const int p = row[k];
        if (covis_point(p, M)) d.mark[p] = 0;
    }
    int fb = 0, top = 0;   // pKFmax (the smallest key among equals); the head of the list at th
    for (int j = tid; j < hi; j += kCovisBlock) {
        const int c = d.votes[j], r = d.rank[j];
        if (c <= 0 || r < 0) continue;
        fb = max(fb, c << kCovisRankBits | (kRankMask - r));
        if (c >= th) top = max(top, c << kCovisRankBits | r);
    }
    fb = block_max(fb, bs, 0);
    top = block_max(top, bs, 1);
    if (fb == 0) {   // `if(KFcounter.empty()) return;`
        if (tid == 0) {
            res[0] = 0;
            res[1] = -1;
        }
        return;
    }
    const int fj = top ? -1 : d.by_rank[kRankMask - (fb & kRankMask)];
    uint16_t* wi = d.W + (size_t)i * Ws;
    for (int j = tid; j < hi; j += kCovisBlock) {
        const int c = d.votes[j];
        wi[j] = (uint16_t)c;   // mConnectedKeyFrameWeights = KFcounter: the entries below th too
        if (c > 0 && (top ? c >= th : j == fj)) {   // AddConnection(j <- i, c)
            uint16_t* wji = d.W + (size_t)j * Ws + i;
            if (*wji != c) {
                *wji = (uint16_t)c;
                d.filt[j] = 0;   // UpdateBestCovisibles: the whole row of j
            }
        }
    }
    if (tid == 0) {
        d.filt[i] = 1;
        d.th[i] = th;
        res[0] = 1;
        res[1] = top ? d.by_rank[top & kRankMask] : fj;
    }
}

// The connection part of KeyFrame::SetBadFlag, entry j of row id (thread 0 of
// the call takes the keyframe's own words as well).
__device__ inline void covis_erase_kf_entry(const CovisDev& d, int hi, int Ws, int id, int j)
{
    if (j == 0) {
        d.row_n[id] = -1;
        d.filt[id] = 0;
        d.th[id] = 0;
    }
    if (j >= hi) return;
    uint16_t* wij = d.W + (size_t)id * Ws + j;
    if (*wij == 0) return;
    uint16_t* wji = d.W + (size_t)j * Ws + id;
    if (*wji != 0) {   // EraseConnection
        *wji = 0;
        d.filt[j] = 0;
    }
    *wij = 0;
}

__global__ __launch_bounds__(kCovisThreads) void k_covis_erase_kf(CovisDev d, int hi, int Ws, int id)
{
    covis_erase_kf_entry(d, hi, Ws, id, blockIdx.x * kCovisThreads + threadIdx.x);
}

__global__ void k_covis_add_kf(CovisDev d, int id, int n)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        d.row_n[id] = n;
        d.filt[id] = 0;
        d.th[id] = 0;
    }
}

// erase_points: pts[0, np) marked, cells[0, nc) (id << 16 | index) cleared.
__global__ __launch_bounds__(kCovisThreads) void k_covis_erase_points(CovisDev d, int P, const int32_t* pts, int np,
                                                                      const int32_t* cells, int nc)
{
    const int t = blockIdx.x * kCovisThreads + threadIdx.x;
    if (t < np) d.erased[pts[t]] = 1;
    if (t < nc) {
        const uint32_t c = (uint32_t)cells[t];
        d.rows[(size_t)(c >> 16) * P + (c & 0xFFFFu)] = -1;
    }
}

// Bitonic sort of keys[0, N) (N a power of two), ascending.
__device__ inline void covis_block_sort(uint32_t* keys, int N)
{
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < N / 2; t += kCovisBlock) {
                const int lo = 2 * t - (t & (j - 1)), hi = lo + j;
                const uint32_t a = keys[lo], c = keys[hi];
                const bool up = (lo & k) == 0;
                if ((a > c) == up) {
                    keys[lo] = c;
                    keys[hi] = a;
                }
            }
            __syncthreads();
        }
}

// The ordered list of member id (which = ORBX_COVIS_ORDERED) or its whole row
// in ascending key order.  Dynamic LDS: N words, N >= hi a power of two.
// res: the length, cap keyframes, cap weights.
__global__ __launch_bounds__(kCovisBlock) void k_covis_list(CovisDev d, int hi, int Ws, int id, int which, int N,
                                                            int32_t* res, int cap)
{
    extern __shared__ uint32_t s_keys[];
    __shared__ BlockScratchN<kCovisBlock / 64> bs;
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const bool ordered = which == ORBX_COVIS_ORDERED;
    const uint16_t* w = d.W + (size_t)id * Ws;
    const int th = (ordered && d.filt[id]) ? d.th[id] : 1;
    if (tid == 0) s_n = 0;
    __syncthreads();
    int fb = 0;
    for (int j = tid; j < hi; j += kCovisBlock) {
        const uint32_t x = w[j];
        const int r = d.rank[j];
        if (x == 0 || r < 0) continue;
        fb = max(fb, (int)(x << kCovisRankBits) | (kRankMask - r));
        // descending (weight, key) as an ascending word; ascending key
        if ((int)x >= th) s_keys[atomicAdd(&s_n, 1)] = ordered ? ~(x << kCovisRankBits | (uint32_t)r) : ((uint32_t)r << 16 | x);
    }
    fb = block_max(fb, bs, 0);   // a barrier: the keys and their count are written
    const int n = s_n;
    if (n == 0) {
        if (tid == 0) {
            res[0] = fb ? 1 : 0;
            if (fb && cap > 0) {   // the fallback entry
                res[1] = d.by_rank[kRankMask - (fb & kRankMask)];
                res[1 + cap] = fb >> kCovisRankBits;
            }
        }
        return;
    }
    for (int k = n + tid; k < N; k += kCovisBlock) s_keys[k] = 0xFFFFFFFFu;
    __syncthreads();
    covis_block_sort(s_keys, N);
    for (int k = tid; k < min(n, cap); k += kCovisBlock) {
        const uint32_t key = ordered ? ~s_keys[k] : s_keys[k];
        res[1 + k] = d.by_rank[ordered ? (key & kRankMask) : (key >> 16)];
        res[1 + cap + k] = (int32_t)(ordered ? (key >> kCovisRankBits) : (key & 0xFFFFu));
    }
    if (tid == 0) res[0] = n;
}

// ---------------------------------------------------------------------------
// LocalMapping::KeyFrameCulling (src/LocalMapping.cc:539-593) and
// MapPointCulling (:190-218).
//
// KeyFrameCulling asks, for every point of a candidate's row, who else observes
// it and at which octave: MapPoint::mObservations.  Here those observer lists
// are gathered for one call, for the points of the candidate rows only:
//
//   k_cull_stamp     mark[p] = 1 for the points of all candidate rows.
//   k_cull_count     one wavefront per member row: mark[p] += 1 per observer.
//   k_cull_offsets   per stamped point one owner (a compare-and-swap on
//                    first[p]) draws a bucket of cells from an atomic cursor,
//                    first[p] = its place, and lists the point.
//   k_cull_fill      the member rows again: every observer's cell (keyframe,
//                    index, octave) into the point's bucket; the slot is what
//                    the atomic decrement of mark[p] returns, so the order in
//                    a bucket is arbitrary, and only counts are taken of it.
//                    mark[p] is back at 1.
//   k_cull_pre       a workgroup per candidate: nMPs and nRedundant against
//                    the state the call found.  They hold until the first cull.
//   k_cull_walk      one workgroup, the candidates in order.  It changes no
//                    lasting state: a culled keyframe is a bit in LDS, a point
//                    that went bad is mark[p] = 2, and the buckets are read
//                    through both, which is the state as the candidates before
//                    left it.  After a cull the counts are taken anew.
//   k_cull_commit    one workgroup: unless a list overflowed its capacity, the
//                    connection part of SetBadFlag for every culled keyframe.
//   k_cull_finish    the listed points: a bad one is marked erased and its
//                    cells cleared from the rows (unless overflowed); mark and
//                    first go back to 0 and ~0.
//
// The launches are the same whatever is culled, and nothing is read back
// before the end.
//
// The predicate.  The reference counts an observation as redundant when, with
// Observations() > 3, its loop over the other observers finds three at an
// octave <= o + 1, and leaves the loop at the third.  Both are shortcuts that
// do not change "at least three such observers": three others and the keyframe
// itself are four observations, so the gate holds whenever the count can reach
// three, and where it fails there are at most two others; the break only stops
// counting once the answer is known.
constexpr int kCullHeader = 8;   // ints: n_cand, n_done, n_bad, commit, cell cursor, n_listed, culls
constexpr int kCullGone = 2;     // mark[p] of a point that a cull of this call erased
constexpr uint32_t kCullClaimed = 0xFFFFFFFEu;

struct CullDev {
    uint64_t* cells;      // per listed point: the number of its cells, then the cells
    int32_t* listed;      // the stamped points, in no order
    int32_t* bad;         // the points the culls erased, in order
    int bad_room;
    int32_t* pre;         // per candidate: nMPs, nRedundant of the state the call found
    int32_t* out;         // kCullHeader ints, then cand, n_mps, n_redundant, decision: stride each
    int stride;
    const int32_t* lst;   // lst[0] candidates lst[1 ...]
    const int32_t* keep;
    int n_keep;
};

__device__ inline uint64_t cull_cell(int kf, int idx, int octave)
{
    return (uint64_t)octave << 32 | (uint32_t)kf << 16 | (uint32_t)idx;
}
__device__ inline int cull_cell_kf(uint64_t c) { return (int)((uint32_t)c >> 16); }
__device__ inline int cull_cell_idx(uint64_t c) { return (int)(c & 0xFFFFu); }
__device__ inline int cull_cell_octave(uint64_t c) { return (int)(c >> 32); }

// candidate k of the list, or -1 where the reference changes nothing: keyframe
// 0, an entry that names no member
__device__ inline int cull_candidate(const CovisDev& d, const CullDev& u, int hi, int k)
{
    const int c = u.lst[1 + k];
    return (c <= 0 || c >= hi || d.row_n[c] < 0) ? -1 : c;
}

__global__ __launch_bounds__(kCovisThreads) void k_cull_stamp(CovisDev d, CullDev u, int hi, int P, int M)
{
    if ((int)blockIdx.x >= u.lst[0]) return;
    const int c = cull_candidate(d, u, hi, blockIdx.x);
    if (c < 0) return;
    const int n = min(d.row_n[c], P);
    const int32_t* row = d.rows + (size_t)c * P;
    for (int i = threadIdx.x; i < n; i += kCovisThreads) {
        const int p = row[i];
        if (covis_point(p, M) && !d.erased[p]) d.mark[p] = 1;
    }
}

// Rows [0, hi), a wavefront each: every entry whose point is stamped adds one
// to the point's mark.
__global__ __launch_bounds__(kCovisThreads) void k_cull_count(CovisDev d, int hi, int P, int M)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * kCovisWaves + (threadIdx.x >> 6);
    if (j >= hi) return;
    const int n = min(d.row_n[j], P);
    const int32_t* row = d.rows + (size_t)j * P;
    for (int i = lane; i < n; i += 64) {
        const int p = row[i];
        if (covis_point(p, M) && d.mark[p] != 0) atomicAdd(&d.mark[p], 1);   // a mark in flight is not 0 either
    }
}

__global__ __launch_bounds__(kCovisThreads) void k_cull_offsets(CovisDev d, CullDev u, int hi, int P, int M)
{
    if ((int)blockIdx.x >= u.lst[0]) return;
    const int c = cull_candidate(d, u, hi, blockIdx.x);
    if (c < 0) return;
    const int n = min(d.row_n[c], P);
    const int32_t* row = d.rows + (size_t)c * P;
    for (int i = threadIdx.x; i < n; i += kCovisThreads) {
        const int p = row[i];
        if (!covis_point(p, M) || d.erased[p]) continue;
        if (atomicCAS(&d.first[p], 0xFFFFFFFFu, kCullClaimed) != 0xFFFFFFFFu) continue;   // another row's thread owns p
        const int cnt = d.mark[p] - 1;
        const uint32_t off = (uint32_t)atomicAdd(&u.out[4], cnt + 1);
        u.cells[off] = (uint64_t)cnt;
        __hip_atomic_store(&d.first[p], off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        u.listed[atomicAdd(&u.out[5], 1)] = p;
    }
}

__global__ __launch_bounds__(kCovisThreads) void k_cull_fill(CovisDev d, CullDev u, int hi, int P, int M)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * kCovisWaves + (threadIdx.x >> 6);
    if (j >= hi) return;
    const int n = min(d.row_n[j], P);
    const int32_t* row = d.rows + (size_t)j * P;
    const uint8_t* oct = d.oct + (size_t)j * P;
    for (int i = lane; i < n; i += 64) {
        const int p = row[i];
        if (!covis_point(p, M) || d.mark[p] == 0) continue;   // it never falls below 1 here
        const int v = atomicSub(&d.mark[p], 1);               // 1 + count ... 2
        const uint32_t off = __hip_atomic_load(&d.first[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        u.cells[(size_t)off + (size_t)(v - 1)] = cull_cell(j, i, oct[i]);
    }
}

__device__ inline bool cull_bit(const uint32_t* bits, int j) { return bits && (bits[j >> 5] >> (j & 31) & 1u); }

// nMPs and nRedundantObservations of candidate c; culled: the keyframes that
// went in this call (a bitmap in LDS), or nullptr.
template <int kT>
__device__ inline void cull_tally(const CovisDev& d, const CullDev& u, int c, int P, int M, const uint32_t* culled,
                                  BlockScratchN<kT / 64>& bs, int* n_mps, int* n_redundant)
{
    const int n = min(d.row_n[c], P);
    const int32_t* row = d.rows + (size_t)c * P;
    const uint8_t* oct = d.oct + (size_t)c * P;
    int mps = 0, red = 0;
    for (int i = threadIdx.x; i < n; i += kT) {
        const int p = row[i];
        if (!covis_point(p, M) || d.erased[p] || d.mark[p] == kCullGone) continue;
        mps++;
        const int o = oct[i];
        const uint64_t* cell = u.cells + d.first[p];
        const int cnt = (int)cell[0];
        int obs = 0;
        for (int t = 1; t <= cnt && obs < 3; t++) {
            const uint64_t x = cell[t];
            const int kf = cull_cell_kf(x);
            if (kf != c && !cull_bit(culled, kf) && cull_cell_octave(x) <= o + 1) obs++;
        }
        red += obs >= 3;
    }
    *n_mps = block_sum(mps, bs, 0);
    *n_redundant = block_sum(red, bs, 1);
}

__global__ __launch_bounds__(kCovisThreads) void k_cull_pre(CovisDev d, CullDev u, int hi, int P, int M)
{
    __shared__ BlockScratchN<kCovisWaves> bs;
    const int k = blockIdx.x;
    if (k >= u.lst[0]) return;
    const int c = cull_candidate(d, u, hi, k);
    int mps = 0, red = 0;
    if (c >= 0) cull_tally<kCovisThreads>(d, u, c, P, M, nullptr, bs, &mps, &red);
    if (threadIdx.x == 0) {
        u.pre[2 * k] = mps;
        u.pre[2 * k + 1] = red;
    }
}

__global__ __launch_bounds__(kCovisBlock) void k_cull_walk(CovisDev d, CullDev u, int hi, int P, int M, int max_culls,
                                                           int cand_cap, int bad_cap)
{
    constexpr int kWords = kCovisMaxKeyframes / 32;
    __shared__ uint32_t s_culled[kWords], s_keep[kWords];
    __shared__ BlockScratchN<kCovisBlock / 64> bs;
    const int tid = threadIdx.x;
    for (int w = tid; w < kWords; w += kCovisBlock) s_culled[w] = s_keep[w] = 0;
    __syncthreads();
    for (int t = tid; t < u.n_keep; t += kCovisBlock) atomicOr(&s_keep[u.keep[t] >> 5], 1u << (u.keep[t] & 31));
    const int n_cand = u.lst[0];
    int32_t* o_cand = u.out + kCullHeader;
    int32_t *o_mps = o_cand + u.stride, *o_red = o_mps + u.stride, *o_dec = o_red + u.stride;
    for (int k = tid; k < n_cand; k += kCovisBlock) o_cand[k] = u.lst[1 + k];
    __syncthreads();
    int n_done = n_cand, n_bad = 0, culls = 0;
    for (int k = 0; k < n_cand; k++) {
        int c = cull_candidate(d, u, hi, k);
        if (c >= 0 && cull_bit(s_culled, c)) c = -1;   // listed twice and gone at its first place
        int mps = 0, red = 0, dec = -1;
        if (c >= 0) {
            if (culls == 0) {
                mps = u.pre[2 * k];
                red = u.pre[2 * k + 1];
            } else {
                cull_tally<kCovisBlock>(d, u, c, P, M, s_culled, bs, &mps, &red);
            }
            // nRedundantObservations > 0.9 * nMPs: one FP64 product, rounded once, and the comparison
            const bool redundant = (double)red > __dmul_rn(0.9, (double)mps);
            dec = !redundant ? 0 : cull_bit(s_keep, c) ? 2 : 1;
        }
        if (tid == 0) {
            o_mps[k] = mps;
            o_red[k] = red;
            o_dec[k] = dec;
        }
        if (dec != 1) continue;
        // MapPoint::EraseObservation for every point of the row: the ones that two keyframes or fewer still
        // hold go bad, in index order
        __syncthreads();   // the tally's reads of the bitmap are done
        if (tid == 0) s_culled[c >> 5] |= 1u << (c & 31);
        __syncthreads();
        const int n = min(d.row_n[c], P);
        const int32_t* row = d.rows + (size_t)c * P;
        int buf = 0;
        for (int i0 = 0; i0 < n; i0 += kCovisBlock, buf ^= 1) {
            const int i = i0 + tid;
            const int p = i < n ? row[i] : -1;
            bool bad = false;
            if (covis_point(p, M) && !d.erased[p] && d.mark[p] != kCullGone) {
                const uint64_t* cell = u.cells + d.first[p];
                const int cnt = (int)cell[0];
                int left = 0;
                for (int t = 1; t <= cnt && left < 3; t++) left += !cull_bit(s_culled, cull_cell_kf(cell[t]));
                bad = left <= 2;
            }
            int total = 0;
            const int o = block_exclusive_scan(bad ? 1 : 0, &total, bs, buf);
            if (bad) {
                d.mark[p] = kCullGone;   // a point stands once in a row: no other thread of this loop reads it
                if (n_bad + o < u.bad_room) u.bad[n_bad + o] = p;
            }
            n_bad += total;
        }
        __syncthreads();   // the marks, before the next candidate's tally
        if (++culls == max_culls) {
            n_done = k + 1;
            break;
        }
    }
    if (tid == 0) {
        u.out[0] = n_cand;
        u.out[1] = n_done;
        u.out[2] = n_bad;
        u.out[3] = (n_cand <= cand_cap && n_bad <= bad_cap) ? 1 : 0;
        u.out[6] = culls;
    }
}

// After k_cull_walk; the culled keyframes one after the other, as
// k_covis_erase_kf takes each.
__global__ __launch_bounds__(kCovisBlock) void k_cull_commit(CovisDev d, CullDev u, int hi, int Ws)
{
    if (!u.out[3]) return;
    const int n_done = u.out[1];
    const int32_t* o_cand = u.out + kCullHeader;
    const int32_t* o_dec = o_cand + 3 * (size_t)u.stride;
    for (int k = 0; k < n_done; k++) {
        if (o_dec[k] != 1) continue;
        for (int j = threadIdx.x; j < max(hi, 1); j += kCovisBlock) covis_erase_kf_entry(d, hi, Ws, o_cand[k], j);
        __syncthreads();   // the next keyframe reads the weights this one wrote
    }
}

__global__ __launch_bounds__(kCovisThreads) void k_cull_finish(CovisDev d, CullDev u, int P)
{
    const int n = u.out[5];
    const bool commit = u.out[3] != 0;
    for (int t = blockIdx.x * kCovisThreads + threadIdx.x; t < n; t += gridDim.x * kCovisThreads) {
        const int p = u.listed[t];
        if (commit && d.mark[p] == kCullGone) {   // MapPoint::SetBadFlag
            d.erased[p] = 1;
            const uint64_t* cell = u.cells + d.first[p];
            const int cnt = (int)cell[0];
            for (int k = 1; k <= cnt; k++) d.rows[(size_t)cull_cell_kf(cell[k]) * P + cull_cell_idx(cell[k])] = -1;
        }
        d.mark[p] = 0;
        d.first[p] = 0xFFFFFFFFu;
    }
}

// MapPointCulling.  in: ids, found, visible, first_kf, n each.  After
// k_cullp_stamp (mark 1) and k_cull_count, mark[p] - 1 is Observations().
__global__ __launch_bounds__(kCovisThreads) void k_cullp_stamp(CovisDev d, const int32_t* in, int n)
{
    const int k = blockIdx.x * kCovisThreads + threadIdx.x;
    if (k < n) d.mark[in[k]] = 1;
}

// The reference's if-chain; mark[p] = -1 for a point that goes, else 0.
__global__ __launch_bounds__(kCovisThreads) void k_cullp_decide(CovisDev d, const int32_t* in, int n, int cur_kf,
                                                                int32_t* action)
{
    const int k = blockIdx.x * kCovisThreads + threadIdx.x;
    if (k >= n) return;
    const int p = in[k], found = in[n + k], visible = in[2 * n + k], age = cur_kf - in[3 * n + k];
    const int observers = d.mark[p] - 1;
    int a = 0;
    if (d.erased[p]) a = 1;
    else if (__fdiv_rn((float)found, (float)visible) < 0.25f) a = 2;   // GetFoundRatio(): FP32, inf and NaN compare false
    else if (age >= 2 && observers <= 2) a = 3;
    else if (age >= 3) a = 4;
    action[k] = a;
    d.mark[p] = (a == 2 || a == 3) ? -1 : 0;
}

// Rows [0, hi), a wavefront each: the cells of the points that go are cleared.
__global__ __launch_bounds__(kCovisThreads) void k_cullp_clear(CovisDev d, int hi, int P, int M)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * kCovisWaves + (threadIdx.x >> 6);
    if (j >= hi) return;
    const int n = min(d.row_n[j], P);
    int32_t* row = d.rows + (size_t)j * P;
    for (int i = lane; i < n; i += 64) {
        const int p = row[i];
        if (covis_point(p, M) && d.mark[p] == -1) row[i] = -1;
    }
}

__global__ __launch_bounds__(kCovisThreads) void k_cullp_finish(CovisDev d, const int32_t* in, int n, const int32_t* action)
{
    const int k = blockIdx.x * kCovisThreads + threadIdx.x;
    if (k >= n || (action[k] != 2 && action[k] != 3)) return;
    d.erased[in[k]] = 1;
    d.mark[in[k]] = 0;
}

}  // namespace orbx

using namespace orbx;

struct orbx_covis {
    int device = 0;
    CovisTable tab;
    int w_stride = 0;
    size_t edit_cap = 0;   // ints of d.edit
    void* mem = nullptr;
    CovisDev d = {};
};

namespace {

bool usable(const orbx_ctx* ctx, const orbx_covis* m) { return ctx && m && m->device == ctx->device; }

int blocks_of(int n) { return (n + kCovisThreads - 1) / kCovisThreads; }

// marks of src[0, n) and the votes of every row below hi
int launch_count(orbx_ctx* ctx, orbx_covis* m, const int32_t* src, int n, int skip, uint8_t* ferased)
{
    const CovisTable& t = m->tab;
    timer_begin(ctx, "covis_count");
    if (n > 0)
        hipLaunchKernelGGL(k_covis_mark, dim3(blocks_of(n)), dim3(kCovisThreads), 0, ctx->stream, m->d, src, n,
                           t.mp_capacity, ferased);
    hipLaunchKernelGGL(k_covis_count, dim3((t.hi + kCovisWaves - 1) / kCovisWaves), dim3(kCovisThreads), 0, ctx->stream,
                       m->d, t.hi, t.max_keypoints, t.mp_capacity, skip);
    timer_end(ctx, "covis_count");
    ORBX_HIP_CHECK(hipGetLastError());
    return ORBX_OK;
}

}  // namespace

extern "C" int orbx_covis_create(orbx_ctx* ctx, int kf_capacity, int mp_capacity, int max_keypoints, orbx_covis** out)
{
    if (!ctx || !out) return ORBX_ERR_ARG;
    *out = nullptr;
    int r = CovisTable::check_create(kf_capacity, mp_capacity, max_keypoints);
    if (r != ORBX_OK) return r;
    orbx_covis* m = new (std::nothrow) orbx_covis;
    if (!m) return ORBX_ERR_NOMEM;
    m->device = ctx->device;
    m->tab.create(kf_capacity, mp_capacity, max_keypoints);
    m->w_stride = (kf_capacity + 7) & ~7;
    m->edit_cap = (size_t)std::max(max_keypoints, 1024) * 2;
    ctx_enter(ctx);
    const size_t K = (size_t)kf_capacity, M = (size_t)mp_capacity, P = (size_t)max_keypoints;
    Layout l;
    const Region<int32_t> o_rows = l.take<int32_t>(K * P), o_rn = l.take<int32_t>(K), o_rank = l.take<int32_t>(K),
                          o_br = l.take<int32_t>(K);
    const Region<uint8_t> o_er = l.take<uint8_t>(M);
    const Region<uint16_t> o_w = l.take<uint16_t>(K * (size_t)m->w_stride);
    const Region<int32_t> o_f = l.take<int32_t>(K), o_th = l.take<int32_t>(K), o_mark = l.take<int32_t>(M);
    const Region<uint32_t> o_first = l.take<uint32_t>(M);
    const Region<int32_t> o_votes = l.take<int32_t>(K);
    const Region<uint8_t> o_incl = l.take<uint8_t>(K);
    const Region<int32_t> o_top = l.take<int32_t>((size_t)kCovisLocalLimit * kCovisBest), o_cnt = l.take<int32_t>(K),
                          o_lkf = l.take<int32_t>(K), o_lmp = l.take<int32_t>(M), o_hdr = l.take<int32_t>(kCovisHeader),
                          o_res = l.take<int32_t>(2 * K + 8), o_edit = l.take<int32_t>(m->edit_cap);
    const Region<uint8_t> o_fe = l.take<uint8_t>(P), o_oct = l.take<uint8_t>(K * P);
    if (hipMalloc(&m->mem, l.total) != hipSuccess) {
        delete m;
        return ORBX_ERR_NOMEM;
    }
    void* b = m->mem;
    m->d = CovisDev{region_ptr(b, o_rows), region_ptr(b, o_rn),   region_ptr(b, o_rank),  region_ptr(b, o_br),
                    region_ptr(b, o_er),   region_ptr(b, o_w),    region_ptr(b, o_f),     region_ptr(b, o_th),
                    region_ptr(b, o_mark), region_ptr(b, o_first), region_ptr(b, o_votes), region_ptr(b, o_incl),
                    region_ptr(b, o_top),  region_ptr(b, o_cnt),  region_ptr(b, o_lkf),   region_ptr(b, o_lmp),
                    region_ptr(b, o_hdr),  region_ptr(b, o_res),  region_ptr(b, o_edit),  region_ptr(b, o_fe),
                    region_ptr(b, o_oct)};
    r = orbx_covis_clear(ctx, m);
    if (r != ORBX_OK) {
        orbx_covis_destroy(m);
        return r;
    }
    *out = m;
    return ORBX_OK;
}

extern "C" void orbx_covis_destroy(orbx_covis* m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->mem) (void)hipFree(m->mem);   // waits for the device's queued work
    delete m;
}

extern "C" int orbx_covis_clear(orbx_ctx* ctx, orbx_covis* m)
{
    if (!usable(ctx, m)) return ORBX_ERR_ARG;
    ctx_enter(ctx);
    const size_t K = (size_t)m->tab.kf_capacity, M = (size_t)m->tab.mp_capacity;
    ORBX_HIP_CHECK(hipMemsetAsync(m->d.row_n, 0xFF, K * sizeof(int32_t), ctx->stream));
    ORBX_HIP_CHECK(hipMemsetAsync(m->d.rank, 0xFF, K * sizeof(int32_t), ctx->stream));
    ORBX_HIP_CHECK(hipMemsetAsync(m->d.by_rank, 0xFF, K * sizeof(int32_t), ctx->stream));
    ORBX_HIP_CHECK(hipMemsetAsync(m->d.erased, 0, M, ctx->stream));
    ORBX_HIP_CHECK(hipMemsetAsync(m->d.W, 0, K * (size_t)m->w_stride * sizeof(uint16_t), ctx->stream));
    ORBX_HIP_CHECK(hipMemsetAsync(m->d.filt, 0, K * sizeof(int32_t), ctx->stream));
    ORBX_HIP_CHECK(hipMemsetAsync(m->d.th, 0, K * sizeof(int32_t), ctx->stream));
    ORBX_HIP_CHECK(hipMemsetAsync(m->d.mark, 0, M * sizeof(int32_t), ctx->stream));
    ORBX_HIP_CHECK(hipMemsetAsync(m->d.first, 0xFF, M * sizeof(uint32_t), ctx->stream));
    ORBX_HIP_CHECK(hipMemsetAsync(m->d.hdr, 0, kCovisHeader * sizeof(int32_t), ctx->stream));
    m->tab.clear();
    return ORBX_OK;
}

extern "C" int orbx_covis_size(const orbx_covis* m) { return m ? m->tab.size : ORBX_ERR_ARG; }

extern "C" int orbx_covis_add_keyframe(orbx_ctx* ctx, orbx_covis* m, int id, uint64_t key, int n, const int32_t* mp)
{
    if (!usable(ctx, m)) return ORBX_ERR_ARG;
    const int r = m->tab.check_add(id, key, n, mp);
    if (r != ORBX_OK) return r;
    ctx_enter(ctx);
    CovisTable& t = m->tab;
    t.commit_add(id, key, n, mp);
    if (n > 0)
        ORBX_HIP_CHECK(hipMemcpyAsync(m->d.rows + (size_t)id * t.max_keypoints, mp, (size_t)n * sizeof(int32_t),
                                      hipMemcpyHostToDevice, ctx->stream));
    // the ranks at and above the new key moved
    const size_t K = (size_t)t.kf_capacity;
    ORBX_HIP_CHECK(hipMemcpyAsync(m->d.rank, t.rank.data(), K * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    ORBX_HIP_CHECK(hipMemcpyAsync(m->d.by_rank, t.by_rank.data(), K * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_covis_add_kf, dim3(1), dim3(64), 0, ctx->stream, m->d, id, n);
    ORBX_HIP_CHECK(hipGetLastError());
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // the caller's row and the shadow are free at return
    return ORBX_OK;
}

extern "C" int orbx_covis_set_matches(orbx_ctx* ctx, orbx_covis* m, int id, int n_edits, const int32_t* idx,
                                      const int32_t* mp)
{
    if (!usable(ctx, m)) return ORBX_ERR_ARG;
    const int r = m->tab.set_matches(id, n_edits, idx, mp);
    if (r != ORBX_OK || n_edits == 0) return r;
    ctx_enter(ctx);
    // the span of the row that the edits touched, from the shadow
    int lo = idx[0], hi = idx[0];
    for (int k = 1; k < n_edits; k++) {
        lo = std::min(lo, idx[k]);
        hi = std::max(hi, idx[k]);
    }
    const std::vector<int32_t>& row = m->tab.rows[(size_t)id];
    ORBX_HIP_CHECK(hipMemcpyAsync(m->d.rows + (size_t)id * m->tab.max_keypoints + lo, row.data() + lo,
                                  (size_t)(hi - lo + 1) * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // the shadow may change after return
    return ORBX_OK;
}

extern "C" int orbx_covis_erase_points(orbx_ctx* ctx, orbx_covis* m, int n, const int32_t* ids)
{
    if (!usable(ctx, m)) return ORBX_ERR_ARG;
    const int r = m->tab.check_points(n, ids);
    if (r != ORBX_OK || n == 0) return r;
    ctx_enter(ctx);
    std::vector<uint32_t> cells;
    m->tab.erase_points(n, ids, cells);
    // chunks of half the edit buffer each: the points in front, the cells behind
    const size_t half = m->edit_cap / 2;
    size_t ip = 0, ic = 0;
    while (ip < (size_t)n || ic < cells.size()) {
        const size_t np = std::min(half, (size_t)n - ip), nc = std::min(half, cells.size() - ic);
        if (np)
            ORBX_HIP_CHECK(hipMemcpyAsync(m->d.edit, ids + ip, np * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        if (nc)
            ORBX_HIP_CHECK(hipMemcpyAsync(m->d.edit + half, cells.data() + ic, nc * sizeof(int32_t), hipMemcpyHostToDevice,
                                          ctx->stream));
        hipLaunchKernelGGL(k_covis_erase_points, dim3(blocks_of((int)std::max(np, nc))), dim3(kCovisThreads), 0,
                           ctx->stream, m->d, m->tab.max_keypoints, m->d.edit, (int)np, m->d.edit + half, (int)nc);
        ORBX_HIP_CHECK(hipGetLastError());
        ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // the chunk's arrays are read
        ip += np;
        ic += nc;
    }
    return ORBX_OK;
}

extern "C" int orbx_covis_erase_keyframe(orbx_ctx* ctx, orbx_covis* m, int id)
{
    if (!usable(ctx, m)) return ORBX_ERR_ARG;
    const int r = m->tab.check_erase_keyframe(id);
    if (r != ORBX_OK) return r;
    ctx_enter(ctx);
    hipLaunchKernelGGL(k_covis_erase_kf, dim3(blocks_of(m->tab.hi)), dim3(kCovisThreads), 0, ctx->stream, m->d,
                       m->tab.hi, m->w_stride, id);
    ORBX_HIP_CHECK(hipGetLastError());
    m->tab.commit_erase_keyframe(id);
    return ORBX_OK;
}

extern "C" int orbx_covis_update_connections(orbx_ctx* ctx, orbx_covis* m, int n, const int32_t* ids, int th,
                                             int32_t* updated, int32_t* front)
{
    if (!usable(ctx, m) || th < 1 || (n > 0 && (!updated || !front))) return ORBX_ERR_ARG;
    int r = m->tab.check_members(n, ids);
    if (r != ORBX_OK || n == 0) return r;
    ctx_enter(ctx);
    const CovisTable& t = m->tab;
    const int chunk = t.kf_capacity;   // ids that d.res holds
    std::vector<int32_t> h((size_t)std::min(n, chunk) * 2);
    for (int k0 = 0; k0 < n; k0 += chunk) {
        const int nk = std::min(chunk, n - k0);
        for (int k = 0; k < nk; k++) {
            const int i = ids[k0 + k];
            const int len = (int)t.rows[(size_t)i].size();
            if ((r = launch_count(ctx, m, m->d.rows + (size_t)i * t.max_keypoints, len, i, nullptr)) != ORBX_OK) return r;
            timer_begin(ctx, "covis_connect");
            hipLaunchKernelGGL(k_covis_connect, dim3(1), dim3(kCovisBlock), 0, ctx->stream, m->d, t.hi, m->w_stride,
                               t.max_keypoints, t.mp_capacity, i, th, m->d.res + 2 * k);
            timer_end(ctx, "covis_connect");
            ORBX_HIP_CHECK(hipGetLastError());
        }
        ORBX_HIP_CHECK(hipMemcpyAsync(h.data(), m->d.res, (size_t)nk * 2 * sizeof(int32_t), hipMemcpyDeviceToHost,
                                      ctx->stream));
        ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        for (int k = 0; k < nk; k++) {
            updated[k0 + k] = h[(size_t)2 * k];
            front[k0 + k] = h[(size_t)2 * k + 1];
        }
    }
    return ORBX_OK;
}

extern "C" int orbx_covis_connections(orbx_ctx* ctx, orbx_covis* m, int id, int which, int32_t* kfs, int32_t* weights,
                                      int cap, int* n)
{
    if (!usable(ctx, m) || !n || cap < 0 || (cap > 0 && (!kfs || !weights)) ||
        (which != ORBX_COVIS_ORDERED && which != ORBX_COVIS_ALL) || !m->tab.is_member(id))
        return ORBX_ERR_ARG;
    *n = 0;
    ctx_enter(ctx);
    const int hi = m->tab.hi;
    const int dcap = std::min(cap, m->tab.kf_capacity);   // a row has at most that many entries
    const int N = covis_sort_len(hi);
    hipLaunchKernelGGL(k_covis_list, dim3(1), dim3(kCovisBlock), (size_t)N * sizeof(uint32_t), ctx->stream, m->d, hi,
                       m->w_stride, id, which, N, m->d.res, dcap);
    ORBX_HIP_CHECK(hipGetLastError());
    std::vector<int32_t> h((size_t)1 + 2 * (size_t)dcap);
    ORBX_HIP_CHECK(hipMemcpyAsync(h.data(), m->d.res, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *n = h[0];
    const int got = std::min(*n, dcap);
    for (int k = 0; k < got; k++) {
        kfs[k] = h[(size_t)1 + k];
        weights[k] = h[(size_t)1 + dcap + k];
    }
    return *n > cap ? ORBX_ERR_CAPACITY : ORBX_OK;
}

extern "C" int orbx_covis_update_reference(orbx_ctx* ctx, orbx_covis* m, orbx_covis_reference_args* q)
{
    if (!usable(ctx, m) || !q || q->kf_cap < 0 || q->mp_cap < 0 || (q->kf_cap > 0 && !q->local_kf) ||
        (q->mp_cap > 0 && !q->local_mp) || !m->tab.frame_ok(q->n, q->frame_mp))
        return ORBX_ERR_ARG;
    q->n_local_kf = q->n_voters = q->n_local_mp = 0;
    q->ref_kf = -1;
    const CovisTable& t = m->tab;
    const int n = q->n;
    if (t.hi == 0) {   // no keyframe was ever added: no row to scan, the flags from the shadow
        if (q->frame_erased)
            for (int i = 0; i < n; i++) q->frame_erased[i] = q->frame_mp[i] >= 0 && t.erased[(size_t)q->frame_mp[i]];
        return ORBX_OK;
    }
    ctx_enter(ctx);
    int r;
    if (n > 0)
        ORBX_HIP_CHECK(hipMemcpyAsync(m->d.edit, q->frame_mp, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if ((r = launch_count(ctx, m, m->d.edit, n, -1, m->d.ferased)) != ORBX_OK) return r;
    const int nr = (int)t.sorted_keys.size();
    timer_begin(ctx, "covis_select");
    hipLaunchKernelGGL(k_covis_select, dim3(1), dim3(kCovisBlock), (size_t)nr * sizeof(int32_t), ctx->stream, m->d, t.hi,
                       nr, m->d.edit, n, t.mp_capacity);
    hipLaunchKernelGGL(k_covis_top, dim3(kCovisLocalLimit), dim3(kCovisThreads), 0, ctx->stream, m->d, t.hi, m->w_stride);
    hipLaunchKernelGGL(k_covis_pass, dim3(1), dim3(64), 0, ctx->stream, m->d, t.hi);
    timer_end(ctx, "covis_select");
    ORBX_HIP_CHECK(hipGetLastError());
    if (t.size > 0) {   // a workgroup per list position; the list is no longer than the members
        timer_begin(ctx, "covis_points");
        hipLaunchKernelGGL(k_covis_first, dim3(t.size), dim3(kCovisThreads), 0, ctx->stream, m->d, t.max_keypoints,
                           t.mp_capacity);
        hipLaunchKernelGGL(k_covis_tally, dim3(t.size), dim3(kCovisThreads), 0, ctx->stream, m->d, t.max_keypoints,
                           t.mp_capacity);
        hipLaunchKernelGGL(k_covis_emit, dim3(t.size), dim3(kCovisThreads), 0, ctx->stream, m->d, t.max_keypoints,
                           t.mp_capacity);
        timer_end(ctx, "covis_points");
        ORBX_HIP_CHECK(hipGetLastError());
    }
    int32_t hdr[4];
    ORBX_HIP_CHECK(hipMemcpyAsync(hdr, m->d.hdr, sizeof(hdr), hipMemcpyDeviceToHost, ctx->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    q->n_local_kf = hdr[0];
    q->n_voters = hdr[1];
    q->ref_kf = hdr[2];
    q->n_local_mp = hdr[3];
    const int nk = std::min(q->n_local_kf, q->kf_cap), np = std::min(q->n_local_mp, q->mp_cap);
    if (nk > 0)
        ORBX_HIP_CHECK(hipMemcpyAsync(q->local_kf, m->d.lkf, (size_t)nk * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (np > 0)
        ORBX_HIP_CHECK(hipMemcpyAsync(q->local_mp, m->d.lmp, (size_t)np * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (q->frame_erased && n > 0)
        ORBX_HIP_CHECK(hipMemcpyAsync(q->frame_erased, m->d.ferased, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return (q->n_local_kf > q->kf_cap || q->n_local_mp > q->mp_cap) ? ORBX_ERR_CAPACITY : ORBX_OK;
}

extern "C" int orbx_covis_set_octaves(orbx_ctx* ctx, orbx_covis* m, int id, int n, const uint8_t* octave)
{
    if (!usable(ctx, m)) return ORBX_ERR_ARG;
    const int r = m->tab.check_octaves(id, n, octave);
    if (r != ORBX_OK) return r;
    ctx_enter(ctx);
    if (n > 0) {
        ORBX_HIP_CHECK(hipMemcpyAsync(m->d.oct + (size_t)id * m->tab.max_keypoints, octave, (size_t)n, hipMemcpyHostToDevice,
                                      ctx->stream));
        ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // the caller's array is free at return
    }
    m->tab.commit_octaves(id);
    return ORBX_OK;
}

extern "C" int orbx_covis_cull_keyframes(orbx_ctx* ctx, orbx_covis* m, orbx_covis_cull_args* q)
{
    if (!usable(ctx, m)) return ORBX_ERR_ARG;
    CovisTable& t = m->tab;
    int r = t.check_cull(q);
    if (r == ORBX_ERR_CAPACITY) {   // the caller's own list does not fit its capacity
        q->n_done = q->n_bad = 0;
        return r;
    }
    if (r != ORBX_OK) return r;
    const bool own = q->cur >= 0;   // the list is cur's, taken on the device
    if (own) q->n_cand = 0;
    q->n_done = q->n_bad = 0;
    if (!own && (q->n_cand == 0 || t.hi == 0)) {   // nothing listed, or no keyframe was ever added: no member to judge
        for (int k = 0; k < q->n_cand; k++) {
            q->n_mps[k] = q->n_redundant[k] = 0;
            q->decision[k] = -1;
        }
        q->n_done = q->n_cand;
        return ORBX_OK;
    }
    ctx_enter(ctx);
    const int hi = t.hi, P = t.max_keypoints, M = t.mp_capacity;
    const int stride = own ? hi : q->n_cand;   // an ordered list names ids below hi, each once
    const size_t cells = t.member_cells();     // every observer cell, every listed point and every bad point is one
    Layout l;
    const Region<uint64_t> o_cells = l.take<uint64_t>(2 * cells + 1);
    const Region<int32_t> o_listed = l.take<int32_t>(cells), o_bad = l.take<int32_t>(cells),
                          o_pre = l.take<int32_t>(2 * (size_t)stride),
                          o_out = l.take<int32_t>(kCullHeader + 4 * (size_t)stride),
                          o_up = l.take<int32_t>(1 + (size_t)(own ? 0 : q->n_cand) + (size_t)q->n_keep);
    if ((r = ensure_scratch(ctx, l.total)) != ORBX_OK) return r;
    void* b = ctx->scratch;
    int32_t* up = region_ptr(b, o_up);
    CullDev u{};
    u.cells = region_ptr(b, o_cells);
    u.listed = region_ptr(b, o_listed);
    u.bad = region_ptr(b, o_bad);
    u.bad_room = (int)cells;   // at most kCovisMaxKeyframes x kCovisMaxKeypoints, below 2^30
    u.pre = region_ptr(b, o_pre);
    u.out = region_ptr(b, o_out);
    u.stride = stride;
    u.n_keep = q->n_keep;
    // one upload: the caller's list behind its length, then the kept keyframes
    std::vector<int32_t> h;
    h.reserve(o_up.count);
    h.push_back(own ? 0 : q->n_cand);
    if (!own) h.insert(h.end(), q->cand, q->cand + q->n_cand);
    u.keep = up + h.size();
    if (q->n_keep) h.insert(h.end(), q->keep, q->keep + q->n_keep);
    ORBX_HIP_CHECK(hipMemcpyAsync(up, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    ORBX_HIP_CHECK(hipMemsetAsync(u.out, 0, kCullHeader * sizeof(int32_t), ctx->stream));
    timer_begin(ctx, "covis_cull_kf");
    if (own) {
        const int N = covis_sort_len(hi);
        hipLaunchKernelGGL(k_covis_list, dim3(1), dim3(kCovisBlock), (size_t)N * sizeof(uint32_t), ctx->stream, m->d, hi,
                           m->w_stride, q->cur, ORBX_COVIS_ORDERED, N, m->d.res, t.kf_capacity);
        u.lst = m->d.res;
    } else {
        u.lst = up;
    }
    const dim3 per_cand(stride), per_row((hi + kCovisWaves - 1) / kCovisWaves), threads(kCovisThreads);
    hipLaunchKernelGGL(k_cull_stamp, per_cand, threads, 0, ctx->stream, m->d, u, hi, P, M);
    hipLaunchKernelGGL(k_cull_count, per_row, threads, 0, ctx->stream, m->d, hi, P, M);
    hipLaunchKernelGGL(k_cull_offsets, per_cand, threads, 0, ctx->stream, m->d, u, hi, P, M);
    hipLaunchKernelGGL(k_cull_fill, per_row, threads, 0, ctx->stream, m->d, u, hi, P, M);
    hipLaunchKernelGGL(k_cull_pre, per_cand, threads, 0, ctx->stream, m->d, u, hi, P, M);
    hipLaunchKernelGGL(k_cull_walk, dim3(1), dim3(kCovisBlock), 0, ctx->stream, m->d, u, hi, P, M, q->max_culls,
                       q->cand_cap, q->bad_cap);
    hipLaunchKernelGGL(k_cull_commit, dim3(1), dim3(kCovisBlock), 0, ctx->stream, m->d, u, hi, m->w_stride);
    const int listed_blocks = std::max(1, std::min(1024, blocks_of(u.bad_room)));   // a grid-stride loop over the list
    hipLaunchKernelGGL(k_cull_finish, dim3(listed_blocks), threads, 0, ctx->stream, m->d, u, P);
    timer_end(ctx, "covis_cull_kf");
    ORBX_HIP_CHECK(hipGetLastError());
    // one read-back of the header and the per-candidate lists; the bad points, whose number the header gives,
    // follow only when a cull took some with it
    std::vector<int32_t> out(o_out.count);
    ORBX_HIP_CHECK(hipMemcpyAsync(out.data(), u.out, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const int n_cand = out[0], n_done = out[1], n_bad = out[2];
    std::vector<int32_t> bad((size_t)n_bad);
    if (n_bad > 0) {
        ORBX_HIP_CHECK(hipMemcpyAsync(bad.data(), u.bad, bad.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    const int32_t* cand = out.data() + kCullHeader;
    const int32_t *mps = cand + stride, *red = mps + stride, *dec = red + stride;
    q->n_cand = n_cand;
    q->n_done = n_done;
    q->n_bad = n_bad;
    for (int k = 0; k < std::min(n_cand, q->cand_cap); k++)
        if (own) q->cand[k] = cand[k];
    for (int k = 0; k < std::min(n_done, q->cand_cap); k++) {
        q->n_mps[k] = mps[k];
        q->n_redundant[k] = red[k];
        q->decision[k] = dec[k];
    }
    for (int k = 0; k < std::min(n_bad, q->bad_cap); k++) q->bad_points[k] = bad[(size_t)k];
    // the shadow follows what the device committed
    r = t.apply_cull(n_cand, q->cand_cap, n_done, cand, dec, n_bad, q->bad_cap, bad.data());
    if (r == ORBX_ERR_CAPACITY) return r;
    return (r == ORBX_OK && out[3] == 1) ? ORBX_OK : ORBX_ERR_HIP;   // the two never differ
}

extern "C" int orbx_covis_cull_points(orbx_ctx* ctx, orbx_covis* m, int cur_kf, int n, const int32_t* ids,
                                      const int32_t* found, const int32_t* visible, const int32_t* first_kf,
                                      int32_t* action)
{
    if (!usable(ctx, m)) return ORBX_ERR_ARG;
    CovisTable& t = m->tab;
    int r = t.check_cull_points(cur_kf, n, ids, found, visible, first_kf, action);
    if (r != ORBX_OK || n == 0) return r;
    ctx_enter(ctx);
    const int hi = t.hi, P = t.max_keypoints, M = t.mp_capacity;
    Layout l;
    const Region<int32_t> o_in = l.take<int32_t>(4 * (size_t)n), o_act = l.take<int32_t>((size_t)n);
    if ((r = ensure_scratch(ctx, l.total)) != ORBX_OK) return r;
    int32_t* in = region_ptr(ctx->scratch, o_in);
    int32_t* act = region_ptr(ctx->scratch, o_act);
    std::vector<int32_t> h;   // one upload
    h.reserve(o_in.count);
    for (const int32_t* a : {ids, found, visible, first_kf}) h.insert(h.end(), a, a + n);
    ORBX_HIP_CHECK(hipMemcpyAsync(in, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const dim3 per_id(blocks_of(n)), per_row((hi + kCovisWaves - 1) / kCovisWaves), threads(kCovisThreads);
    timer_begin(ctx, "covis_cull_mp");
    hipLaunchKernelGGL(k_cullp_stamp, per_id, threads, 0, ctx->stream, m->d, in, n);
    if (hi > 0) hipLaunchKernelGGL(k_cull_count, per_row, threads, 0, ctx->stream, m->d, hi, P, M);
    hipLaunchKernelGGL(k_cullp_decide, per_id, threads, 0, ctx->stream, m->d, in, n, cur_kf, act);
    if (hi > 0) hipLaunchKernelGGL(k_cullp_clear, per_row, threads, 0, ctx->stream, m->d, hi, P, M);
    hipLaunchKernelGGL(k_cullp_finish, per_id, threads, 0, ctx->stream, m->d, in, n, act);
    timer_end(ctx, "covis_cull_mp");
    ORBX_HIP_CHECK(hipGetLastError());
    ORBX_HIP_CHECK(hipMemcpyAsync(action, act, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    t.apply_cull_points(n, ids, action);
    return ORBX_OK;
}
