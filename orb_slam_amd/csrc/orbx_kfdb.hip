// KeyFrameDatabase on MI355X: the keyframes' BowVectors in HBM and
// DetectRelocalisationCandidates / DetectLoopCandidates
// (src/KeyFrameDatabase.cc:75-308) as two kernels per query.
//
// The reference walks an inverted file (a std::list<KeyFrame*> per word) to
// count the words each keyframe shares with the query, then calls
// L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) for every
// keyframe that shares enough.  Here the members' BowVectors lie row by row
// (words ascending, as the std::map iterates) and a query scans all of them:
//
//   k_kfdb_scan    one wavefront per member.  The query sits in LDS; the lanes
//                  stride over the member's words, binary-search the query and
//                  ballot the hits.  The popcount is mn*Words, the first hit
//                  the smallest common word, and the FP64 terms of the hit
//                  lanes are added one after the other in lane order (a
//                  readlane walk over the mask), which is the order of the
//                  reference's merge loop: ascending common words.
//   k_kfdb_select  one workgroup.  maxCommonWords over the sharing list, the
//                  word and score gates, the sharing list's order, the
//                  covisibility accumulation, the 0.75 threshold and the
//                  ordered, de-duplicated output.
//
// List order.  lKFsSharingWords is filled while the query's words are walked
// ascending and each word's list in add() order, so a member's place is given
// by (its smallest common word, its add sequence number): a 64-bit key, sorted
// in LDS.  Every later list of the reference is a filtered copy in that order.
#include <climits>
#include <cmath>
#include <new>
#include <vector>

#include "orbx_device.h"
#include "orbx_internal.h"
#include "orbx_kfdb_host.h"
#include "orbx_stage.h"

namespace orbx {

// flags[m] of one query
constexpr int kKfExcluded = 1;   // named by the caller's exclude list (scan)
constexpr int kKfListed = 2;     // in lKFsSharingWords
constexpr int kKfGate = 4;       // words > minCommonWords (scored)
constexpr int kKfMatch = 8;      // in lScoreAndMatch

struct KfdbDev {
    // members: capacity rows of max_words entries
    uint32_t* words;
    double* values;
    int32_t* n_words;      // -1: the id is free
    uint32_t* seq;         // add sequence number
    int32_t* neigh;        // capacity x 10, -1 padded
    float* reloc_score;    // mRelocScore
    // the running query, per id
    int32_t* cw;           // common words
    uint32_t* fw;          // smallest common word
    float* sc;             // score of the query against the member
    int32_t* flags;
    float* acc;
    int32_t* best;
    int32_t* pos;          // position in the sharing list
    int32_t* minpos;       // first list position whose pBestKF is this id
    int32_t* at_pos;       // list position -> the id emitted there
    int32_t* tap_words;
    float* tap_score;
};

constexpr int kScanThreads = 256;
constexpr int kSelectThreads = 1024;
constexpr int kResHeader = 8;   // ints in front of the candidates

// One member's metadata at add (n >= 0) or erase (n = -1).
__global__ void k_kfdb_meta(KfdbDev d, int id, int n, uint32_t seq)
{
    const int t = threadIdx.x;
    if (t < kKfdbNeigh) d.neigh[id * kKfdbNeigh + t] = -1;
    if (t == 0) {
        d.n_words[id] = n;
        d.seq[id] = seq;
        d.reloc_score[id] = 0.0f;
    }
}

// add from a slot: the count is the slot's (clamped to the row), read here.
__global__ __launch_bounds__(256) void k_kfdb_add_slot(KfdbDev d, int id, int W, uint32_t seq, const uint32_t* sw,
                                                       const double* sv, const int32_t* sn)
{
    const int n = min(max(*sn, 0), W);
    uint32_t* w = d.words + (size_t)id * W;
    double* v = d.values + (size_t)id * W;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        w[i] = sw[i];
        v[i] = sv[i];
    }
    if (threadIdx.x < kKfdbNeigh) d.neigh[id * kKfdbNeigh + threadIdx.x] = -1;
    if (threadIdx.x == 0) {
        d.n_words[id] = n;
        d.seq[id] = seq;
        d.reloc_score[id] = 0.0f;
    }
}

__global__ void k_kfdb_neigh(KfdbDev d, int n, const int32_t* ids, const int32_t* rows)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * kKfdbNeigh) d.neigh[ids[i / kKfdbNeigh] * kKfdbNeigh + i % kKfdbNeigh] = rows[i];
}

// Members [0, hi), a wavefront each.  Dynamic LDS: q_cap doubles, q_cap words.
// The query's length is nq_host, or *nq_dev for a slot query; at most q_cap
// entries of it are used.
__global__ __launch_bounds__(kScanThreads) void k_kfdb_scan(KfdbDev d, int hi, int W, const uint32_t* qw,
                                                            const double* qv, const int32_t* nq_dev, int nq_host,
                                                            int q_cap, const int32_t* excl, int n_excl)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    double* s_v = reinterpret_cast<double*>(smem);
    uint32_t* s_w = reinterpret_cast<uint32_t*>(smem + (size_t)q_cap * sizeof(double));
    const int nq = min(max(nq_dev ? *nq_dev : nq_host, 0), q_cap);
    for (int i = threadIdx.x; i < nq; i += kScanThreads) {
        s_v[i] = qv[i];
        s_w[i] = qw[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * (kScanThreads / 64) + (threadIdx.x >> 6);
    if (m >= hi) return;
    const int n = min(d.n_words[m], W);
    if (n < 0) {
        if (lane == 0) {
            d.cw[m] = 0;
            d.fw[m] = 0xFFFFFFFFu;
            d.sc[m] = 0.0f;
            d.flags[m] = 0;
        }
        return;
    }
    bool ex = false;
    for (int i = lane; i < n_excl; i += 64) ex = ex || excl[i] == m;
    const bool excluded = __ballot(ex) != 0ull;

    const uint32_t* mw = d.words + (size_t)m * W;
    const double* mv = d.values + (size_t)m * W;
    double sum = 0.0;   // L1Scoring::score's `score`, the same value in every lane
    int cnt = 0;
    uint32_t first = 0xFFFFFFFFu;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool hit = false;
        uint32_t w = 0;
        double term = 0.0;
        if (i < n) {
            w = mw[i];
            int lo = 0, up = nq;
            while (lo < up) {
                const int mid = (lo + up) >> 1;
                if (s_w[mid] < w) lo = mid + 1;
                else up = mid;
            }
            if (lo < nq && s_w[lo] == w) {
                hit = true;
                const double vi = s_v[lo], wi = mv[i];   // v1 is the query, v2 the member
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);
            }
        }
        unsigned long long mask = __ballot(hit);
        if (mask == 0ull) continue;
        if (cnt == 0) first = (uint32_t)__builtin_amdgcn_readlane((int)w, __builtin_ctzll(mask));
        cnt += __popcll(mask);
        while (mask) {   // ascending lanes are ascending words: the reference's chain of additions
            sum += readlane_f64(term, __builtin_ctzll(mask));
            mask &= mask - 1;
        }
    }
    if (lane == 0) {
        d.cw[m] = cnt;
        d.fw[m] = first;
        d.sc[m] = (float)(-sum / 2.0);   // `float si = mpVoc->score(...)`
        d.flags[m] = excluded ? kKfExcluded : 0;
    }
}

// Bitonic sort of keys[0, N) (N a power of two) by the block
// (orbx_vocab.hip's block sort, on this kernel's thread count).
__device__ inline void kfdb_block_sort(uint64_t* keys, int N)
{
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < N / 2; t += kSelectThreads) {
                const int lo = 2 * t - (t & (j - 1)), hi = lo + j;
                const uint64_t a = keys[lo], c = keys[hi];
                const bool up = (lo & k) == 0;
                if ((a > c) == up) {
                    keys[lo] = c;
                    keys[hi] = a;
                }
            }
            __syncthreads();
        }
}

// kMin: `if (s < v) v = s` over the block; else `if (s > v) v = s`.  Both are
// exact in any order.  Two barriers; s_f holds a float per wave.
template <bool kMin>
__device__ inline float kfdb_block_pick(float v, float* s_f)
{
    for (int o = 32; o > 0; o >>= 1) {
        const float s = __shfl_xor(v, o, 64);
        if (kMin ? s < v : s > v) v = s;
    }
    __syncthreads();   // s_f free again
    if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = s_f[0];
    for (int i = 1; i < kSelectThreads / 64; i++) {
        const float s = s_f[i];
        if (kMin ? s < r : s > r) r = s;
    }
    return r;
}

// After k_kfdb_scan.  Dynamic LDS: sort_cap 64-bit keys, sort_cap >= the
// members below hi rounded up to a power of two.  res: kResHeader ints
// (n_candidates, min_score_used, max_common_words, n_scored, n_sharing), then
// cap candidates.
__global__ __launch_bounds__(kSelectThreads) void k_kfdb_select(KfdbDev d, int hi, int mode, float min_score,
                                                                const int32_t* ref, int n_ref, int sort_cap,
                                                                int32_t* res, int cap)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t s_keys[];
    __shared__ BlockScratchN<kSelectThreads / 64> bs;
    __shared__ float s_f[kSelectThreads / 64];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const bool loop = mode == ORBX_KFDB_LOOP;

    // DetectLoop's minScore (src/LoopClosing.cc:124-136), from the scan's scores
    float ms = 0.0f;
    if (loop) {
        float v = min_score;
        for (int i = tid; i < n_ref; i += kSelectThreads) {
            const int r = ref[i];
            if (r >= 0 && r < hi && d.n_words[r] >= 0) {
                const float s = d.sc[r];
                if (s < v) v = s;
            }
        }
        ms = kfdb_block_pick<true>(v, s_f);
    }

    // the sharing list and maxCommonWords over it
    int lmax = 0, lcnt = 0;
    for (int m = tid; m < hi; m += kSelectThreads) {
        const int c = d.n_words[m] >= 0 ? d.cw[m] : 0;
        int f = d.flags[m] & kKfExcluded;
        if (c > 0 && !(loop && f)) {
            f |= kKfListed;
            lmax = max(lmax, c);
            lcnt++;
        }
        d.flags[m] = f;
        d.acc[m] = 0.0f;
        d.best[m] = -1;
        d.pos[m] = -1;
        d.minpos[m] = INT_MAX;
        d.at_pos[m] = -1;
    }
    if (tid == 0) s_n = 0;
    const int maxc = block_max(lmax, bs, 0);
    const int nl = block_sum(lcnt, bs, 1);   // <= sort_cap: the listed are members below hi
    const int minc = (int)((float)maxc * 0.8f);   // `int minCommonWords = maxCommonWords*0.8f;`

    // the gates, mRelocScore, the list's keys
    int nsc = 0;
    for (int m = tid; m < hi; m += kSelectThreads) {
        int f = d.flags[m];
        const float s = d.sc[m];
        float ts = 0.0f;
        if (f & kKfListed) {
            if (d.cw[m] > minc) {
                f |= kKfGate;
                nsc++;
                if (!loop) d.reloc_score[m] = s;
                if (!loop || s >= ms) f |= kKfMatch;
                ts = s;
            }
            d.flags[m] = f;
            s_keys[atomicAdd(&s_n, 1)] = (uint64_t)d.fw[m] << 32 | d.seq[m];
        }
        const bool member = d.n_words[m] >= 0;
        d.tap_words[m] = (f & kKfListed) ? d.cw[m] : 0;
        d.tap_score[m] = loop ? ts : (member ? d.reloc_score[m] : 0.0f);
    }
    int N = 2;
    while (N < nl) N <<= 1;
    N = min(N, sort_cap);
    for (int i = nl + tid; i < N; i += kSelectThreads) s_keys[i] = ~0ull;
    const int n_scored = block_sum(nsc, bs, 0);   // a barrier: keys and flags are written
    kfdb_block_sort(s_keys, N);
    for (int m = tid; m < hi; m += kSelectThreads) {
        if (!(d.flags[m] & kKfListed)) continue;
        const uint64_t key = (uint64_t)d.fw[m] << 32 | d.seq[m];
        int lo = 0, up = nl;
        while (lo < up) {   // keys are unique: the sequence numbers are
            const int mid = (lo + up) >> 1;
            if (s_keys[mid] < key) lo = mid + 1;
            else up = mid;
        }
        d.pos[m] = min(lo, nl - 1);
    }
    __syncthreads();

    // accumulation over GetBestCovisibilityKeyFrames(10), bestAccScore
    float bacc = loop ? ms : 0.0f;
    for (int m = tid; m < hi; m += kSelectThreads) {
        if (!(d.flags[m] & kKfMatch)) continue;
        const float si = d.sc[m];
        float best_score = si, acc = si;
        int best = m;
        for (int k = 0; k < kKfdbNeigh; k++) {
            const int nb = d.neigh[m * kKfdbNeigh + k];
            if (nb < 0 || nb >= hi || d.n_words[nb] < 0) continue;
            float s2;
            if (loop) {   // mnLoopQuery == this query && mnLoopWords > minCommonWords
                if (!(d.flags[nb] & kKfGate)) continue;
                s2 = d.sc[nb];
            } else {      // mnRelocQuery == this query: it shares a word
                if (d.cw[nb] <= 0) continue;
                s2 = d.reloc_score[nb];
            }
            acc += s2;
            if (s2 > best_score) {
                best = nb;
                best_score = s2;
            }
        }
        d.acc[m] = acc;
        d.best[m] = best;
        if (acc > bacc) bacc = acc;
    }
    bacc = kfdb_block_pick<false>(bacc, s_f);
    const float retain = 0.75f * bacc;

    // first occurrence of every pBestKF, in list order
    for (int m = tid; m < hi; m += kSelectThreads)
        if ((d.flags[m] & kKfMatch) && d.acc[m] > retain) atomicMin(&d.minpos[d.best[m]], d.pos[m]);
    __syncthreads();
    for (int m = tid; m < hi; m += kSelectThreads) {
        // written by atomics, which act in L2: read it there
        const int p = __hip_atomic_load(&d.minpos[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p != INT_MAX) d.at_pos[p] = m;   // a position has one member, a member one pBestKF
    }
    __syncthreads();
    const int per = (nl + kSelectThreads - 1) / kSelectThreads;
    const int p0 = min(tid * per, nl), p1 = min(p0 + per, nl);
    int mine = 0;
    for (int p = p0; p < p1; p++) mine += d.at_pos[p] >= 0;
    int total = 0;
    int o = block_exclusive_scan(mine, &total, bs, 1);
    for (int p = p0; p < p1; p++) {
        const int b = d.at_pos[p];
        if (b < 0) continue;
        if (o < cap) res[kResHeader + o] = b;
        o++;
    }
    if (tid == 0) {
        res[0] = total;
        res[1] = __float_as_int(ms);
        res[2] = maxc;
        res[3] = n_scored;
        res[4] = nl;
    }
}

}  // namespace orbx

using namespace orbx;

struct orbx_kfdb {
    int device = 0;
    KfdbTable tab;
    void* mem = nullptr;
    KfdbDev d = {};
};

namespace {

// The query's BowVector on the device: a slot's arrays, or regions of the
// call's packed upload.
struct QuerySource {
    const uint32_t* w = nullptr;
    const double* v = nullptr;
    const int32_t* n_dev = nullptr;
    int n_host = 0;
    int q_cap = 1;   // LDS entries of the scan
};

bool slot_has_bow(const orbx_ctx* ctx, int slot)
{
    return slot >= 0 && slot < ctx->slots && ctx->bow_dev && slot < (int)ctx->bow_ready.size() && ctx->bow_ready[slot];
}

// Argument checks of a query's BowVector; takes the host arrays' regions.
int stage_query_bow(orbx_ctx* ctx, const orbx_kfdb* db, int slot, int n_words, const uint32_t* words,
                    const double* values, PackedStage& st, Region<double>& r_v, Region<uint32_t>& r_w)
{
    if (slot >= 0) {
        if (!slot_has_bow(ctx, slot)) return ORBX_ERR_ARG;
        if (db->tab.max_words < ctx->bow_nf) return ORBX_ERR_CAPACITY;
        return ORBX_OK;
    }
    if (slot != -1 || !KfdbTable::bow_ok(n_words, words, values)) return ORBX_ERR_ARG;
    if (n_words > db->tab.max_words) return ORBX_ERR_CAPACITY;
    r_v = st.take<double>((size_t)n_words, values);
    r_w = st.take<uint32_t>((size_t)n_words, words);
    return ORBX_OK;
}

QuerySource query_source(orbx_ctx* ctx, int slot, int n_words, const PackedStage& st, Region<double> r_v,
                         Region<uint32_t> r_w)
{
    QuerySource s;
    if (slot >= 0) {
        const size_t o = (size_t)slot * ctx->bow_nf;
        s.w = ctx->bow.bow_words + o;
        s.v = ctx->bow.bow_values + o;
        s.n_dev = ctx->bow.counts + 2 * slot;
        s.q_cap = std::max(ctx->bow_nf, 1);
    } else {
        s.w = st.dev(r_w);
        s.v = st.dev(r_v);
        s.n_host = n_words;
        s.q_cap = std::max(n_words, 1);
    }
    return s;
}

int launch_scan(orbx_ctx* ctx, orbx_kfdb* db, const QuerySource& s, const int32_t* excl, int n_excl)
{
    const int hi = db->tab.hi;
    if (hi <= 0) return ORBX_OK;
    const int waves = kScanThreads / 64;
    const size_t lds = (size_t)s.q_cap * (sizeof(double) + sizeof(uint32_t));
    timer_begin(ctx, "kfdb_scan");
    hipLaunchKernelGGL(k_kfdb_scan, dim3((hi + waves - 1) / waves), dim3(kScanThreads), lds, ctx->stream, db->d, hi,
                       db->tab.max_words, s.w, s.v, s.n_dev, s.n_host, s.q_cap, excl, n_excl);
    timer_end(ctx, "kfdb_scan");
    ORBX_HIP_CHECK(hipGetLastError());
    return ORBX_OK;
}

bool usable(const orbx_ctx* ctx, const orbx_kfdb* db) { return ctx && db && db->device == ctx->device; }

}  // namespace

extern "C" int orbx_kfdb_create(orbx_ctx* ctx, int capacity, int max_words, orbx_kfdb** out)
{
    if (!ctx || !out) return ORBX_ERR_ARG;
    *out = nullptr;
    int r = KfdbTable::check_create(capacity, max_words);
    if (r != ORBX_OK) return r;
    orbx_kfdb* db = new (std::nothrow) orbx_kfdb;
    if (!db) return ORBX_ERR_NOMEM;
    db->device = ctx->device;
    db->tab.create(capacity, max_words);
    ctx_enter(ctx);
    const size_t C = (size_t)capacity, rows = C * (size_t)max_words;
    Layout l;
    const Region<double> o_v = l.take<double>(rows);
    const Region<uint32_t> o_w = l.take<uint32_t>(rows);
    const Region<int32_t> o_n = l.take<int32_t>(C);
    const Region<uint32_t> o_seq = l.take<uint32_t>(C);
    const Region<int32_t> o_ng = l.take<int32_t>(C * kKfdbNeigh);
    const Region<float> o_rs = l.take<float>(C);
    const Region<int32_t> o_cw = l.take<int32_t>(C);
    const Region<uint32_t> o_fw = l.take<uint32_t>(C);
    const Region<float> o_sc = l.take<float>(C);
    const Region<int32_t> o_fl = l.take<int32_t>(C);
    const Region<float> o_acc = l.take<float>(C);
    const Region<int32_t> o_best = l.take<int32_t>(C), o_pos = l.take<int32_t>(C), o_mp = l.take<int32_t>(C),
                          o_at = l.take<int32_t>(C), o_tw = l.take<int32_t>(C);
    const Region<float> o_ts = l.take<float>(C);
    if (hipMalloc(&db->mem, l.total) != hipSuccess) {
        delete db;
        return ORBX_ERR_NOMEM;
    }
    void* m = db->mem;
    db->d = KfdbDev{region_ptr(m, o_w),   region_ptr(m, o_v),   region_ptr(m, o_n),  region_ptr(m, o_seq),
                    region_ptr(m, o_ng),  region_ptr(m, o_rs),  region_ptr(m, o_cw), region_ptr(m, o_fw),
                    region_ptr(m, o_sc),  region_ptr(m, o_fl),  region_ptr(m, o_acc), region_ptr(m, o_best),
                    region_ptr(m, o_pos), region_ptr(m, o_mp),  region_ptr(m, o_at), region_ptr(m, o_tw),
                    region_ptr(m, o_ts)};
    r = orbx_kfdb_clear(ctx, db);
    if (r != ORBX_OK) {
        orbx_kfdb_destroy(db);
        return r;
    }
    *out = db;
    return ORBX_OK;
}

extern "C" void orbx_kfdb_destroy(orbx_kfdb* db)
{
    if (!db) return;
    (void)hipSetDevice(db->device);
    if (db->mem) (void)hipFree(db->mem);   // waits for the device's queued work
    delete db;
}

extern "C" int orbx_kfdb_clear(orbx_ctx* ctx, orbx_kfdb* db)
{
    if (!usable(ctx, db)) return ORBX_ERR_ARG;
    ctx_enter(ctx);
    const size_t C = (size_t)db->tab.capacity;
    // every id free (n_words -1), every neighbour row -1, every score 0
    ORBX_HIP_CHECK(hipMemsetAsync(db->d.n_words, 0xFF, C * sizeof(int32_t), ctx->stream));
    ORBX_HIP_CHECK(hipMemsetAsync(db->d.neigh, 0xFF, C * kKfdbNeigh * sizeof(int32_t), ctx->stream));
    ORBX_HIP_CHECK(hipMemsetAsync(db->d.reloc_score, 0, C * sizeof(float), ctx->stream));
    db->tab.clear();
    return ORBX_OK;
}

extern "C" int orbx_kfdb_size(const orbx_kfdb* db) { return db ? db->tab.size : ORBX_ERR_ARG; }

extern "C" int orbx_kfdb_add(orbx_ctx* ctx, orbx_kfdb* db, int id, int n_words, const uint32_t* words,
                             const double* values)
{
    if (!usable(ctx, db) || !KfdbTable::bow_ok(n_words, words, values)) return ORBX_ERR_ARG;
    const int r = db->tab.check_add(id, n_words);
    if (r != ORBX_OK) return r;
    ctx_enter(ctx);
    const size_t o = (size_t)id * db->tab.max_words;
    if (n_words > 0) {
        ORBX_HIP_CHECK(hipMemcpyAsync(db->d.words + o, words, (size_t)n_words * sizeof(uint32_t),
                                      hipMemcpyHostToDevice, ctx->stream));
        ORBX_HIP_CHECK(hipMemcpyAsync(db->d.values + o, values, (size_t)n_words * sizeof(double),
                                      hipMemcpyHostToDevice, ctx->stream));
    }
    hipLaunchKernelGGL(k_kfdb_meta, dim3(1), dim3(64), 0, ctx->stream, db->d, id, n_words, db->tab.next_seq);
    ORBX_HIP_CHECK(hipGetLastError());
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // the caller's arrays are free at return
    db->tab.commit_add(id);
    return ORBX_OK;
}

extern "C" int orbx_kfdb_add_slot(orbx_ctx* ctx, orbx_kfdb* db, int id, int slot)
{
    if (!usable(ctx, db) || !slot_has_bow(ctx, slot)) return ORBX_ERR_ARG;
    const int r = db->tab.check_add(id, ctx->bow_nf);   // a slot holds at most nfeatures words
    if (r != ORBX_OK) return r;
    ctx_enter(ctx);
    const size_t o = (size_t)slot * ctx->bow_nf;
    hipLaunchKernelGGL(k_kfdb_add_slot, dim3(1), dim3(256), 0, ctx->stream, db->d, id, db->tab.max_words,
                       db->tab.next_seq, ctx->bow.bow_words + o, ctx->bow.bow_values + o, ctx->bow.counts + 2 * slot);
    ORBX_HIP_CHECK(hipGetLastError());
    db->tab.commit_add(id);
    return ORBX_OK;
}

extern "C" int orbx_kfdb_erase(orbx_ctx* ctx, orbx_kfdb* db, int id)
{
    if (!usable(ctx, db)) return ORBX_ERR_ARG;
    const int r = db->tab.check_erase(id);
    if (r != ORBX_OK) return r;
    ctx_enter(ctx);
    hipLaunchKernelGGL(k_kfdb_meta, dim3(1), dim3(64), 0, ctx->stream, db->d, id, -1, 0u);
    ORBX_HIP_CHECK(hipGetLastError());
    db->tab.commit_erase(id);
    return ORBX_OK;
}

extern "C" int orbx_kfdb_set_neighbours(orbx_ctx* ctx, orbx_kfdb* db, int n, const int32_t* ids, const int32_t* neigh)
{
    if (!usable(ctx, db) || (n > 0 && !neigh)) return ORBX_ERR_ARG;
    int r = db->tab.check_members(n, ids);
    if (r != ORBX_OK) return r;
    if (n == 0) return ORBX_OK;
    ctx_enter(ctx);
    PackedStage st(ctx);
    const Region<int32_t> r_ids = st.take<int32_t>((size_t)n, ids);
    const Region<int32_t> r_rows = st.take<int32_t>((size_t)n * kKfdbNeigh, neigh);
    if ((r = st.open(0)) != ORBX_OK || (r = st.upload()) != ORBX_OK) return r;
    const int items = n * kKfdbNeigh;
    hipLaunchKernelGGL(k_kfdb_neigh, dim3((items + 255) / 256), dim3(256), 0, ctx->stream, db->d, n, st.dev(r_ids),
                       st.dev(r_rows));
    ORBX_HIP_CHECK(hipGetLastError());
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // the staged rows live in this call
    return ORBX_OK;
}

extern "C" int orbx_kfdb_query(orbx_ctx* ctx, orbx_kfdb* db, orbx_kfdb_query_args* q)
{
    if (!usable(ctx, db) || !q || (q->mode != ORBX_KFDB_RELOC && q->mode != ORBX_KFDB_LOOP) || q->cap < 0 ||
        (q->cap > 0 && !q->candidates))
        return ORBX_ERR_ARG;
    const bool loop = q->mode == ORBX_KFDB_LOOP;
    const int n_ref = loop ? q->n_ref : 0, n_excl = loop ? q->n_exclude : 0;
    int r;
    if (loop && ((r = db->tab.check_ids(n_ref, q->ref)) != ORBX_OK || (r = db->tab.check_ids(n_excl, q->exclude)) != ORBX_OK))
        return r;
    PackedStage st(ctx);
    Region<double> r_v;
    Region<uint32_t> r_w;
    if ((r = stage_query_bow(ctx, db, q->slot, q->n_words, q->words, q->values, st, r_v, r_w)) != ORBX_OK) return r;
    const Region<int32_t> r_ref = st.take<int32_t>((size_t)n_ref, q->ref);
    const Region<int32_t> r_ex = st.take<int32_t>((size_t)n_excl, q->exclude);

    q->n_candidates = 0;
    q->min_score_used = loop ? q->min_score : 0.0f;
    q->max_common_words = q->n_sharing = q->n_scored = 0;
    const int C = db->tab.capacity, hi = db->tab.hi;
    auto tap_defaults = [&]() {
        for (int i = 0; i < C; i++) {
            if (q->tap_words) q->tap_words[i] = 0;
            if (q->tap_score) q->tap_score[i] = 0.0f;
            if (q->tap_acc) q->tap_acc[i] = 0.0f;
            if (q->tap_best) q->tap_best[i] = -1;
            if (q->tap_pos) q->tap_pos[i] = -1;
        }
    };
    tap_defaults();
    if (db->tab.size == 0) return ORBX_OK;   // an empty inverted file: lKFsSharingWords.empty()

    ctx_enter(ctx);
    const int cap = std::min(q->cap, C);   // a vector of distinct members
    const size_t res_bytes = (size_t)(kResHeader + cap) * sizeof(int32_t);
    if ((r = st.open(res_bytes)) != ORBX_OK || (r = st.upload()) != ORBX_OK) return r;
    const QuerySource src = query_source(ctx, q->slot, q->n_words, st, r_v, r_w);
    if ((r = launch_scan(ctx, db, src, st.dev(r_ex), n_excl)) != ORBX_OK) return r;
    const int sort_cap = kfdb_sort_len(std::min(db->tab.size, hi));
    ResultBlocks res(ctx, st.behind(), 1, res_bytes);
    timer_begin(ctx, "kfdb_select");
    hipLaunchKernelGGL(k_kfdb_select, dim3(1), dim3(kSelectThreads), (size_t)sort_cap * sizeof(uint64_t), ctx->stream,
                       db->d, hi, q->mode, q->min_score, st.dev(r_ref), n_ref, sort_cap,
                       reinterpret_cast<int32_t*>(res.dev), cap);
    timer_end(ctx, "kfdb_select");
    ORBX_HIP_CHECK(hipGetLastError());
    auto tap = [&](void* dst, const void* src_dev) -> int {
        if (dst) ORBX_HIP_CHECK(hipMemcpyAsync(dst, src_dev, (size_t)hi * 4, hipMemcpyDeviceToHost, ctx->stream));
        return ORBX_OK;
    };
    if ((r = tap(q->tap_words, db->d.tap_words)) || (r = tap(q->tap_score, db->d.tap_score)) ||
        (r = tap(q->tap_acc, db->d.acc)) || (r = tap(q->tap_best, db->d.best)) || (r = tap(q->tap_pos, db->d.pos)))
        return r;
    if ((r = res.read()) != ORBX_OK) return r;
    const int32_t* h = reinterpret_cast<const int32_t*>(res.block(0));
    q->n_candidates = h[0];
    std::memcpy(&q->min_score_used, &h[1], sizeof(float));
    if (!loop) q->min_score_used = 0.0f;
    q->max_common_words = h[2];
    q->n_scored = h[3];
    q->n_sharing = h[4];
    const int got = std::min(q->n_candidates, cap);
    if (got > 0) std::memcpy(q->candidates, h + kResHeader, (size_t)got * sizeof(int32_t));
    return q->n_candidates > q->cap ? ORBX_ERR_CAPACITY : ORBX_OK;
}

extern "C" int orbx_kfdb_score(orbx_ctx* ctx, orbx_kfdb* db, int slot, int n_words, const uint32_t* words,
                               const double* values, int n, const int32_t* ids, float* scores)
{
    if (!usable(ctx, db) || (n > 0 && !scores)) return ORBX_ERR_ARG;
    int r = db->tab.check_members(n, ids);
    if (r != ORBX_OK) return r;
    PackedStage st(ctx);
    Region<double> r_v;
    Region<uint32_t> r_w;
    if ((r = stage_query_bow(ctx, db, slot, n_words, words, values, st, r_v, r_w)) != ORBX_OK) return r;
    if (n == 0) return ORBX_OK;
    ctx_enter(ctx);
    const int hi = db->tab.hi;
    if ((r = st.open(0)) != ORBX_OK || (r = st.upload()) != ORBX_OK) return r;
    const QuerySource src = query_source(ctx, slot, n_words, st, r_v, r_w);
    if ((r = launch_scan(ctx, db, src, nullptr, 0)) != ORBX_OK) return r;
    std::vector<float> all((size_t)hi);
    ORBX_HIP_CHECK(hipMemcpyAsync(all.data(), db->d.sc, (size_t)hi * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n; k++) scores[k] = all[(size_t)ids[k]];
    return ORBX_OK;
}
