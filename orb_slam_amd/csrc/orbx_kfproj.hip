// Keyframe projection searches on MI355X: the state-free part of
// ORBmatcher::Fuse (both overloads, src/ORBmatcher.cc:1016-1265),
// SearchBySim3 (:1267-1505) and MapPoint::ComputeDistinctiveDescriptors
// (src/MapPoint.cc:185-250).
//
// Projection: one wavefront per map point, four per 256-thread workgroup.
// The keyframe's keypoint table (position, grid cell, octave) is staged in
// LDS once per workgroup; each wavefront computes its point's projection
// and gates redundantly on every lane (uniform), then the lanes stride the
// keyframe's keypoints with the GetFeaturesInArea cell/box test and the
// level window, and one 64-bit min reduction over (distance, cell, index)
// gives the reference's first strict minimum in GetFeaturesInArea order.
// cv::Mat arithmetic is restated as in oracle/ref_proj.cpp (float products
// summed left to right, scalar scaling by a double factor, cv::norm and
// Mat::dot accumulated in double).
//
// Distinctive descriptors: one wavefront per map point; lane i takes
// descriptor i and finds the median of its distance row by a binary search
// on the value (9 counting passes over the row), then a (median, i) min
// reduction picks the first least median.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "orbx_device.h"
#include "orbx_internal.h"
#include "orbx_match_common.h"
#include "orbx_stage.h"

namespace orbx {

struct KfProjArgs {
    FrameDev K;                 // searched keyframe
    float scales[kMaxLevels];
    int nlevels;
    float cam[4];
    float Ra[9], ta[3];         // p = Ra X + ta
    float Rb[9], tb[3];         // then p = Rb p + tb (two_stage)
    float Ow[3];
    int two_stage;
    int mode;                   // 0 Fuse (1/z float), 1 Fuse Scw (1.0/z double), 2 SearchBySim3
    float th;
    int nq;
    const float* pos;
    const float* normal;
    const float* dmin;
    const float* dmax;
    const uint8_t* qdesc;
    const uint8_t* qvalid;      // may be null
    int32_t* best_idx;
    int32_t* best_dist;
};

__device__ inline void xform3(const float* R, const float* t, const float* X, float* o)
{
#pragma unroll
    for (int r = 0; r < 3; r++)
        o[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[3 * r], X[0]), __fmul_rn(R[3 * r + 1], X[1])),
                                   __fmul_rn(R[3 * r + 2], X[2])),
                         t[r]);
}

__device__ inline float norm3_cv(const float* v)
{
    double s = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) s += (double)v[i] * (double)v[i];
    return (float)sqrt(s);
}

__device__ inline double dot3_cv(const float* a, const float* b)
{
    double s = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) s += (double)a[i] * (double)b[i];
    return s;
}

__device__ inline void kf_project_block(const KfProjArgs& a, uint8_t* smem, int mblock)
{
    float* tx = reinterpret_cast<float*>(smem);
    float* ty = tx + a.K.n;
    int* tco = reinterpret_cast<int*>(ty + a.K.n);   // cell | octave << 16
    for (int i = threadIdx.x; i < a.K.n; i += kBlock) {
        const orbx_keypoint k = a.K.kps[i];
        tx[i] = k.x;
        ty[i] = k.y;
        const int cell = grid_cell(a.K, k.x, k.y);
        tco[i] = (cell & 0xFFFF) | (k.octave << 16);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int m = mblock * (kBlock / 64) + (threadIdx.x >> 6);
    if (m >= a.nq) return;
    int best_idx = -1, best_dist = INT_MAX;
    do {
        if (a.qvalid && !a.qvalid[m]) break;
        const float Xw[3] = {a.pos[3 * m], a.pos[3 * m + 1], a.pos[3 * m + 2]};
        float pc[3];
        xform3(a.Ra, a.ta, Xw, pc);
        if (a.two_stage) {
            const float p1[3] = {pc[0], pc[1], pc[2]};
            xform3(a.Rb, a.tb, p1, pc);
        }
        if (pc[2] < 0.0f) break;
        const float invz = a.mode == 0 ? __fdiv_rn(1.0f, pc[2]) : (float)(1.0 / (double)pc[2]);
        const float x = __fmul_rn(pc[0], invz), y = __fmul_rn(pc[1], invz);
        const float u = __fadd_rn(__fmul_rn(a.cam[0], x), a.cam[2]);
        const float v = __fadd_rn(__fmul_rn(a.cam[1], y), a.cam[3]);
        if (!(u >= a.K.min_x && u < a.K.max_x && v >= a.K.min_y && v < a.K.max_y)) break;   // IsInImage
        const float maxDistance = a.dmax[m], minDistance = a.dmin[m];
        float dist3D;
        if (a.mode == 2) {
            dist3D = norm3_cv(pc);   // SearchBySim3: norm of the camera point
        } else {
            const float PO[3] = {__fsub_rn(Xw[0], a.Ow[0]), __fsub_rn(Xw[1], a.Ow[1]), __fsub_rn(Xw[2], a.Ow[2])};
            dist3D = norm3_cv(PO);
            if (dist3D < minDistance || dist3D > maxDistance) break;
            const float Pn[3] = {a.normal[3 * m], a.normal[3 * m + 1], a.normal[3 * m + 2]};
            if (dot3_cv(PO, Pn) < 0.5 * (double)dist3D) break;
        }
        if (dist3D < minDistance || dist3D > maxDistance) break;
        const float ratio = __fdiv_rn(dist3D, minDistance);
        int pred = 0;
        while (pred < a.nlevels && a.scales[pred] < ratio) pred++;   // lower_bound
        pred = min(pred, a.nlevels - 1);
        const float radius = __fmul_rn(a.th, a.scales[pred]);
        const AreaQuery q = area_cells(a.K, u, v, radius);
        if (q.empty) break;
        uint4 d0, d1;
        load_desc(a.qdesc + (size_t)m * 32, d0, d1);
        unsigned long long bk = ~0ull;
        for (int j = lane; j < a.K.n; j += 64) {
            const int co = tco[j];
            const int oct = co >> 16;
            if (oct < pred - 1 || oct > pred) continue;
            const int cell = (co & 0xFFFF) == 0xFFFF ? -1 : (co & 0xFFFF);
            if (!in_area(q, cell, tx[j], ty[j], u, v, radius)) continue;
            uint4 b0, b1;
            load_desc(a.K.desc + (size_t)j * 32, b0, b1);
            const unsigned long long key = ((unsigned long long)hamming256(d0, d1, b0, b1) << 32) |
                                           ((unsigned long long)cell << 12) | (unsigned long long)j;
            bk = key < bk ? key : bk;
        }
        bk = wave_min_u64(bk);
        if (bk != ~0ull) {
            best_idx = (int)(bk & 0xFFF);
            best_dist = (int)(bk >> 32);
        }
    } while (false);
    if (lane == 0) {
        a.best_idx[m] = best_idx;
        a.best_dist[m] = best_dist;
    }
}

__global__ __launch_bounds__(256) void k_kf_project(KfProjArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    kf_project_block(a, smem, blockIdx.x);
}

// Batched form: grid.y = keyframe job (each with its own keypoint table,
// pose and map points), grid.x = blocks of four map points.
__global__ __launch_bounds__(256) void k_kf_project_jobs(const KfProjArgs* jobs)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const KfProjArgs& a = jobs[blockIdx.y];
    if ((int)blockIdx.x * (kBlock / 64) >= a.nq) return;   // uniform per block
    kf_project_block(a, smem, blockIdx.x);
}

// MapPoint::ComputeDistinctiveDescriptors, one wavefront per map point.
__global__ __launch_bounds__(256) void k_distinctive(const int32_t* ptr, const uint8_t* desc, int n_mp, int32_t* best)
{
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (m >= n_mp) return;
    const int b0 = ptr[m], N = ptr[m + 1] - b0;
    if (N <= 0) {
        if (lane == 0) best[m] = -1;
        return;
    }
    const uint8_t* D = desc + (size_t)b0 * 32;
    const int k = (N - 1) / 2;                     // vDists[0.5*(N-1)]
    uint32_t key = 0xFFFFFFFFu;
    for (int i = lane; i < N; i += 64) {
        uint4 a0, a1;
        load_desc(D + (size_t)i * 32, a0, a1);
        int lo = 0, hi = 256;                       // smallest v with #{d(i,l) <= v} > k
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            int cnt = 0;
            for (int l = 0; l < N; l++) {
                uint4 c0, c1;
                load_desc(D + (size_t)l * 32, c0, c1);
                cnt += hamming256(a0, a1, c0, c1) <= mid;
            }
            if (cnt > k) hi = mid;
            else lo = mid + 1;
        }
        const uint32_t kk = ((uint32_t)lo << 20) | (uint32_t)i;
        key = kk < key ? kk : key;
    }
    key = wave_min_u32(key);
    if (lane == 0) best[m] = (int)(key & 0xFFFFF);
}


// Sequential projection searches (the candidate exclusion depends on the
// earlier points' assignments): one wavefront replays the reference's loop
// over the points in order; per point the lanes stride the searched
// frame's keypoints (LDS table) and one min reduction gives the first
// strict minimum in GetFeaturesInArea order.
//  variant 0: SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th)
//             (src/ORBmatcher.cc:286-407)
//  variant 1: SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th,
//             ORBdist) (:1622-1746), with the rotation-consistency filter
struct SeqProjArgs {
    FrameDev T;                 // searched keyframe (variant 0) / frame (variant 1)
    float scales[kMaxLevels];
    int nlevels;
    float cam[4];
    float R[9], t[3], Ow[3];
    float th;
    int orb_dist, check_ori, variant;
    int nq;
    const float* pos;
    const float* normal;
    const float* dmin;
    const float* dmax;
    const uint8_t* qdesc;
    const uint8_t* qskip;       // variant 0: isBad || already found; variant 1: !valid
    const orbx_keypoint* qkps;  // variant 1: the KF keypoints (angles)
    const uint8_t* assigned;    // variant 1: CurrentFrame.mvpMapPoints[i] != NULL
    int32_t* out;               // variant 0: vpMatched (in/out); variant 1: matches_f
    int32_t* out_n;
};

__global__ __launch_bounds__(64) void k_proj_seq(SeqProjArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int n = a.T.n, lane = threadIdx.x;
    float* tx = reinterpret_cast<float*>(smem);
    float* ty = tx + n;
    int* tco = reinterpret_cast<int*>(ty + n);
    int* taken = tco + n;
    int* keys = taken + n;
    int* hist = keys + n;
    signed char* bins = reinterpret_cast<signed char*>(hist + 32);
    for (int i = lane; i < n; i += 64) {
        const orbx_keypoint k = a.T.kps[i];
        tx[i] = k.x;
        ty[i] = k.y;
        const int cell = grid_cell(a.T, k.x, k.y);
        tco[i] = (cell & 0xFFFF) | (k.octave << 16);
        taken[i] = a.variant == 0 ? (a.out[i] >= 0) : (int)a.assigned[i];
    }
    wave_sync();
    int nmatches = 0, npushed = 0;
    for (int m = 0; m < a.nq; m++) {
        if (a.qskip[m]) continue;
        const float Xw[3] = {a.pos[3 * m], a.pos[3 * m + 1], a.pos[3 * m + 2]};
        float pc[3];
        xform3(a.R, a.t, Xw, pc);
        float u, v;
        int pred, lo, hi, accept;
        const float PO[3] = {__fsub_rn(Xw[0], a.Ow[0]), __fsub_rn(Xw[1], a.Ow[1]), __fsub_rn(Xw[2], a.Ow[2])};
        const float dist3D = norm3_cv(PO);
        const float minDistance = a.dmin[m];
        if (a.variant == 0) {
            if (pc[2] < 0.0f) continue;
            const float invz = __fdiv_rn(1.0f, pc[2]);
            u = __fadd_rn(__fmul_rn(a.cam[0], __fmul_rn(pc[0], invz)), a.cam[2]);
            v = __fadd_rn(__fmul_rn(a.cam[1], __fmul_rn(pc[1], invz)), a.cam[3]);
            if (!(u >= a.T.min_x && u < a.T.max_x && v >= a.T.min_y && v < a.T.max_y)) continue;
            if (dist3D < minDistance || dist3D > a.dmax[m]) continue;
            const float Pn[3] = {a.normal[3 * m], a.normal[3 * m + 1], a.normal[3 * m + 2]};
            if (dot3_cv(PO, Pn) < 0.5 * (double)dist3D) continue;
        } else {
            const float invzc = (float)(1.0 / (double)pc[2]);
            u = __fadd_rn(__fmul_rn(__fmul_rn(a.cam[0], pc[0]), invzc), a.cam[2]);
            v = __fadd_rn(__fmul_rn(__fmul_rn(a.cam[1], pc[1]), invzc), a.cam[3]);
            if (u < a.T.min_x || u > a.T.max_x) continue;
            if (v < a.T.min_y || v > a.T.max_y) continue;
        }
        const float ratio = __fdiv_rn(dist3D, minDistance);
        pred = 0;
        while (pred < a.nlevels && a.scales[pred] < ratio) pred++;
        pred = min(pred, a.nlevels - 1);
        const float radius = __fmul_rn(a.th, a.scales[pred]);
        if (a.variant == 0) {
            lo = pred - 1;
            hi = pred;
            accept = kTHLow;
        } else {
            lo = pred - 1;
            hi = pred + 1;
            accept = a.orb_dist;
        }
        const AreaQuery q = area_cells(a.T, u, v, radius);
        if (q.empty) continue;
        uint4 d0, d1;
        load_desc(a.qdesc + (size_t)m * 32, d0, d1);
        unsigned long long bk = ~0ull;
        for (int j = lane; j < n; j += 64) {
            const int co = tco[j];
            const int oct = co >> 16;
            if (oct < lo || oct > hi) continue;
            const int cell = (co & 0xFFFF) == 0xFFFF ? -1 : (co & 0xFFFF);
            if (!in_area(q, cell, tx[j], ty[j], u, v, radius)) continue;
            if (taken[j]) continue;
            uint4 b0, b1;
            load_desc(a.T.desc + (size_t)j * 32, b0, b1);
            const unsigned long long key = ((unsigned long long)hamming256(d0, d1, b0, b1) << 32) |
                                           ((unsigned long long)cell << 12) | (unsigned long long)j;
            bk = key < bk ? key : bk;
        }
        bk = wave_min_u64(bk);
        if (bk == ~0ull || (int)(bk >> 32) > accept) continue;
        const int j = (int)(bk & 0xFFF);
        if (lane == 0) {
            taken[j] = 1;
            a.out[j] = m;
            if (a.variant == 1 && a.check_ori) {
                bins[npushed] = (signed char)rot_bin(a.qkps[m].angle, a.T.kps[j].angle);
                keys[npushed] = j;
            }
        }
        if (a.variant == 1 && a.check_ori) npushed++;
        nmatches++;
        wave_sync();
    }
    wave_sync();
    if (lane == 0) {
        if (npushed) {
            for (int b = 0; b < kHistoLength; b++) hist[b] = 0;
            for (int i = 0; i < npushed; i++) hist[bins[i]]++;
            int i1, i2, i3;
            three_maxima(hist, i1, i2, i3);
            for (int i = 0; i < npushed; i++) {
                const int b = bins[i];
                if (b == i1 || b == i2 || b == i3) continue;
                a.out[keys[i]] = -1;
                nmatches--;
            }
        }
        *a.out_n = nmatches;
    }
}

namespace {

bool valid_mps(const orbx_mappoint_view* p, bool need_normal)
{
    return p && p->n >= 0 &&
           (p->n == 0 || (p->pos && p->min_dist && p->max_dist && p->desc && (!need_normal || p->normal)));
}

// Same arithmetic as oracle/ref_proj.cpp pose_parts (src/ORBmatcher.cc:
// 1145-1149; KeyFrame::SetPose's Ow = -Rwc * tcw).
void pose_parts(const float* T, int sim3, float* R, float* t, float* Ow)
{
    if (sim3) {
        double s = 0;
        for (int c = 0; c < 3; c++) s += (double)T[c] * (double)T[c];
        const float scw = (float)std::sqrt(s);
        const double inv = 1.0 / (double)scw;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) R[3 * r + c] = (float)((double)T[4 * r + c] * inv);
            t[r] = (float)((double)T[4 * r + 3] * inv);
        }
    } else {
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) R[3 * r + c] = T[4 * r + c];
            t[r] = T[4 * r + 3];
        }
    }
    for (int c = 0; c < 3; c++) Ow[c] = -(R[c] * t[0] + R[3 + c] * t[1] + R[6 + c] * t[2]);
}

// The slot's count as the device holds it, at most nfeatures.
int slot_count(const orbx_ctx* ctx, int32_t cnt) { return std::min<int>(cnt, ctx->geom.nfeatures); }

// The frame in `slot` with the bounds the kfproj calls document: the
// caller's, or 0..w x 0..h.
FrameDev kf_slot_dev(const orbx_ctx* ctx, int slot, const float* bounds, int n)
{
    const float image[4] = {0.f, (float)ctx->geom.w, 0.f, (float)ctx->geom.h};
    FrameDev F = slot_frame_dev(ctx, slot, bounds ? bounds : image);
    F.n = n;
    return F;
}

struct KfRegions {
    Region<orbx_keypoint> kp;
    Region<uint8_t> kd;
};

KfRegions take_kf(ArrayStage& s, const orbx_frame_view* K)
{
    KfRegions o;
    o.kp = s.take((size_t)K->n, K->keys_un);
    o.kd = s.take((size_t)K->n * 32, K->desc);
    return o;
}

struct MpRegions {
    Region<float> pos, nrm, dmin, dmax;
    Region<uint8_t> qd;
};

MpRegions take_mps(ArrayStage& s, const orbx_mappoint_view* P)
{
    MpRegions o;
    o.pos = s.take((size_t)P->n * 3, P->pos);
    o.nrm = s.take((size_t)P->n * 3, P->normal);
    o.dmin = s.take((size_t)P->n, P->min_dist);
    o.dmax = s.take((size_t)P->n, P->max_dist);
    o.qd = s.take((size_t)P->n * 32, P->desc);
    return o;
}

// KfProjArgs and SeqProjArgs name the map-point arrays alike.
template <typename Args>
void set_mps(Args& a, const ArrayStage& s, const MpRegions& o, int nq)
{
    a.nq = nq;
    a.pos = s.dev(o.pos);
    a.normal = s.dev(o.nrm);
    a.dmin = s.dev(o.dmin);
    a.dmax = s.dev(o.dmax);
    a.qdesc = s.dev(o.qd);
}

// Stages the keyframe and the map points, fills the common fields.
struct ProjStage {
    KfRegions k;
    MpRegions mp;
    Region<uint8_t> qv;
    Region<int32_t> bi, bd;
};

ProjStage stage_proj(ArrayStage& s, const orbx_frame_view* K, const orbx_mappoint_view* P, const uint8_t* qvalid)
{
    ProjStage o;
    o.k = take_kf(s, K);
    o.mp = take_mps(s, P);
    o.qv = s.take((size_t)P->n, qvalid);
    o.bi = s.take<int32_t>(P->n);
    o.bd = s.take<int32_t>(P->n);
    return o;
}

// One projection job of keyframe K (n levels of scale_factor) over nq points.
void fill_job(KfProjArgs& a, const ArrayStage& s, const FrameDev& K, int nlevels, float scale_factor,
              const MpRegions& mp, int nq, Region<int32_t> bi, Region<int32_t> bd)
{
    a.K = K;
    a.nlevels = nlevels;
    level_scales(nlevels, scale_factor, a.scales);
    set_mps(a, s, mp, nq);
    a.best_idx = s.dev(bi);
    a.best_dist = s.dev(bd);
}

void fill_proj(KfProjArgs& a, const ArrayStage& s, const ProjStage& o, const orbx_frame_view* K,
               const orbx_mappoint_view* P, bool has_valid)
{
    fill_job(a, s, frame_dev(K, s.dev(o.k.kp), s.dev(o.k.kd)), K->nlevels, K->scale_factor, o.mp, P->n, o.bi, o.bd);
    a.qvalid = has_valid ? s.dev(o.qv) : nullptr;
}

// Fuse's job k of a batch: camera, pose and threshold.
void set_fuse(KfProjArgs& a, const float* cam, const float* T, int sim3, float th)
{
    for (int c = 0; c < 4; c++) a.cam[c] = cam[c];
    pose_parts(T, sim3, a.Ra, a.ta, a.Ow);
    a.two_stage = 0;
    a.mode = sim3 ? 1 : 0;
    a.th = th;
}

// A fuse batch's tail: the job table up, one launch, each job's two result
// arrays straight into the caller's.
struct FuseOut {
    Region<int32_t> bi, bd;
};
int run_fuse_jobs(ArrayStage& s, const std::vector<KfProjArgs>& jobs, Region<KfProjArgs> o_jobs, int max_q, int max_n,
                  const std::vector<FuseOut>& o, int32_t* const* best_idx, int32_t* const* best_dist)
{
    orbx_ctx* ctx = s.ctx;
    s.later(o_jobs, jobs.data());
    int r = s.upload();
    if (r != ORBX_OK) return r;
    if (max_q > 0) {
        const int per = kBlock / 64;
        hipLaunchKernelGGL(k_kf_project_jobs, dim3((max_q + per - 1) / per, (unsigned)jobs.size()), dim3(kBlock),
                           (size_t)max_n * 12, ctx->stream, s.dev(o_jobs));
        ORBX_HIP_CHECK(hipGetLastError());
    }
    for (size_t k = 0; k < jobs.size(); k++)
        if ((r = s.get(best_idx[k], o[k].bi)) || (r = s.get(best_dist[k], o[k].bd))) return r;
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return ORBX_OK;
}

// The map points of job k: those of an earlier job that passed the same view
// (uploaded once), else staged here.
MpRegions take_shared_mps(ArrayStage& s, const orbx_mappoint_view* const* mps, const std::vector<MpRegions>& mp, int k)
{
    for (int j = 0; j < k; j++)
        if (mps[j] == mps[k]) return mp[j];
    return take_mps(s, mps[k]);
}

// k_proj_seq over the frame a.T, then its matches (n of them) and their
// count into the caller's memory.
int run_proj_seq(ArrayStage& s, SeqProjArgs& a, Region<int32_t> out, Region<int32_t> out_n, int32_t* matches,
                 int* n_matches)
{
    orbx_ctx* ctx = s.ctx;
    a.out = s.dev(out);
    a.out_n = s.dev(out_n);
    const size_t lds = (size_t)std::max(a.T.n, 1) * 21 + 32 * 4 + 64;
    hipLaunchKernelGGL(k_proj_seq, dim3(1), dim3(64), lds, ctx->stream, a);
    ORBX_HIP_CHECK(hipGetLastError());
    int r;
    if ((r = s.get(matches, out, a.T.n)) || (r = s.get(n_matches, out_n))) return r;
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return ORBX_OK;
}

// What the sequential searches set alike: the searched frame, its pyramid,
// camera and pose.
void set_seq(SeqProjArgs& a, const FrameDev& T, int nlevels, float scale_factor, const float* cam, const float* pose,
             int sim3, float th, int variant)
{
    a.T = T;
    a.nlevels = nlevels;
    level_scales(nlevels, scale_factor, a.scales);
    for (int k = 0; k < 4; k++) a.cam[k] = cam[k];
    pose_parts(pose, sim3, a.R, a.t, a.Ow);
    a.th = th;
    a.variant = variant;
}

int launch_proj(orbx_ctx* ctx, const KfProjArgs& a)
{
    if (a.nq == 0) return ORBX_OK;
    const int per = kBlock / 64;
    const size_t lds = (size_t)std::max(a.K.n, 1) * 12;
    hipLaunchKernelGGL(k_kf_project, dim3((a.nq + per - 1) / per), dim3(kBlock), lds, ctx->stream, a);
    ORBX_HIP_CHECK(hipGetLastError());
    return ORBX_OK;
}

}  // namespace
}  // namespace orbx

using namespace orbx;

extern "C" int orbx_fuse_candidates(orbx_ctx* ctx, const orbx_frame_view* KF, const float* cam,
                                    const orbx_mappoint_view* mps, const float* T, int sim3, float th,
                                    int32_t* best_idx, int32_t* best_dist)
{
    if (!ctx || !valid_frame_view(KF) || !cam || !valid_mps(mps, true) || !T ||
        (mps->n > 0 && (!best_idx || !best_dist)))
        return ORBX_ERR_ARG;
    ctx_enter(ctx);
    ArrayStage s(ctx);
    const ProjStage o = stage_proj(s, KF, mps, nullptr);
    int r = s.upload();
    if (r != ORBX_OK) return r;
    KfProjArgs a{};
    fill_proj(a, s, o, KF, mps, false);
    set_fuse(a, cam, T, sim3, th);
    if ((r = launch_proj(ctx, a)) != ORBX_OK) return r;
    if ((r = s.get(best_idx, o.bi)) || (r = s.get(best_dist, o.bd))) return r;
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return ORBX_OK;
}

// SearchInNeighbors' first loop (src/LocalMapping.cc:403-416: Fuse of the
// current keyframe's map points into every target keyframe) in one upload,
// one launch and one readback.  Map-point views that are the same object are
// uploaded once.
extern "C" int orbx_fuse_candidates_batch(orbx_ctx* ctx, int n_kf, const orbx_frame_view* KFs, const float* cams,
                                          const orbx_mappoint_view* const* mps, const float* Ts, int sim3, float th,
                                          int32_t* const* best_idx, int32_t* const* best_dist)
{
    if (!ctx || n_kf < 0 || (n_kf > 0 && (!KFs || !cams || !mps || !Ts || !best_idx || !best_dist))) return ORBX_ERR_ARG;
    for (int k = 0; k < n_kf; k++)
        if (!valid_frame_view(&KFs[k]) || !valid_mps(mps[k], true) || (mps[k]->n > 0 && (!best_idx[k] || !best_dist[k])))
            return ORBX_ERR_ARG;
    if (n_kf == 0) return ORBX_OK;
    ctx_enter(ctx);
    ArrayStage s(ctx);
    std::vector<KfRegions> kf(n_kf);
    std::vector<MpRegions> mp(n_kf);
    std::vector<FuseOut> o(n_kf);
    int max_n = 1, max_q = 0;
    for (int k = 0; k < n_kf; k++) {
        kf[k] = take_kf(s, &KFs[k]);
        mp[k] = take_shared_mps(s, mps, mp, k);
        o[k].bi = s.take<int32_t>(mps[k]->n);
        o[k].bd = s.take<int32_t>(mps[k]->n);
        max_n = std::max(max_n, KFs[k].n);
        max_q = std::max(max_q, mps[k]->n);
    }
    const Region<KfProjArgs> o_jobs = s.take<KfProjArgs>(n_kf);
    std::vector<KfProjArgs> jobs(n_kf);
    const int r = s.open();
    if (r != ORBX_OK) return r;
    for (int k = 0; k < n_kf; k++) {
        const orbx_frame_view* K = &KFs[k];
        fill_job(jobs[k], s, frame_dev(K, s.dev(kf[k].kp), s.dev(kf[k].kd)), K->nlevels, K->scale_factor, mp[k],
                 mps[k]->n, o[k].bi, o[k].bd);
        set_fuse(jobs[k], cams + 4 * k, Ts + 16 * k, sim3, th);
    }
    return run_fuse_jobs(s, jobs, o_jobs, max_q, max_n, o, best_idx, best_dist);
}

// LocalMapping::SearchInNeighbors' Fuse loop against keyframes that stay in
// their extraction slots: the keyframes' keypoints (mvKeysUn after
// orbx_dev_undistort) and descriptors are read where orbx_dev_extract left
// them; only the map points, poses and cameras travel.
extern "C" int orbx_dev_fuse_candidates(orbx_ctx* ctx, int n_kf, const int* slots, const float* bounds,
                                        const float* cams, const orbx_mappoint_view* const* mps, const float* Ts,
                                        int sim3, float th, int32_t* const* best_idx, int32_t* const* best_dist)
{
    if (!ctx || n_kf < 0 || (n_kf > 0 && (!slots || !cams || !mps || !Ts || !best_idx || !best_dist)))
        return ORBX_ERR_ARG;
    if (ctx->geom_w <= 0) return ORBX_ERR_ARG;
    for (int k = 0; k < n_kf; k++) {
        if (slots[k] < 0 || slots[k] >= ctx->slots || !valid_mps(mps[k], true) ||
            (mps[k]->n > 0 && (!best_idx[k] || !best_dist[k])))
            return ORBX_ERR_ARG;
        if (bounds && !(bounds[4 * k + 1] > bounds[4 * k] && bounds[4 * k + 3] > bounds[4 * k + 2])) return ORBX_ERR_ARG;
    }
    if (n_kf == 0) return ORBX_OK;
    ctx_enter(ctx);
    // the slots' keypoint counts size the kernel's LDS grid
    std::vector<int32_t> cnt;
    if (const int rc = read_slot_counts(ctx, cnt)) return rc;
    const Geometry& g = ctx->geom;
    ArrayStage s(ctx);
    std::vector<MpRegions> mp(n_kf);
    std::vector<FuseOut> o(n_kf);
    int max_n = 1, max_q = 0;
    for (int k = 0; k < n_kf; k++) {
        mp[k] = take_shared_mps(s, mps, mp, k);
        o[k].bi = s.take<int32_t>(mps[k]->n);
        o[k].bd = s.take<int32_t>(mps[k]->n);
        max_n = std::max(max_n, slot_count(ctx, cnt[slots[k]]));
        max_q = std::max(max_q, mps[k]->n);
    }
    const Region<KfProjArgs> o_jobs = s.take<KfProjArgs>(n_kf);
    std::vector<KfProjArgs> jobs(n_kf);
    const int r = s.open();
    if (r != ORBX_OK) return r;
    for (int k = 0; k < n_kf; k++) {
        // the extracted frame as a keyframe (bounds: the caller's
        // ComputeImageBounds, or the undistorted image 0..w, 0..h)
        const FrameDev K = kf_slot_dev(ctx, slots[k], bounds ? bounds + 4 * k : nullptr, slot_count(ctx, cnt[slots[k]]));
        fill_job(jobs[k], s, K, g.nlevels, g.scale_factor, mp[k], mps[k]->n, o[k].bi, o[k].bd);
        set_fuse(jobs[k], cams + 4 * k, Ts + 16 * k, sim3, th);
    }
    return run_fuse_jobs(s, jobs, o_jobs, max_q, max_n, o, best_idx, best_dist);
}

// SearchBySim3 for keyframe views whose keypoints and descriptors are on
// the host (dev1 / dev2 null: staged) or already on the device (the slot
// arrays: the views then carry only counts, bounds and the scale pyramid).
static int run_sim3(orbx_ctx* ctx, const orbx_frame_view* KF1, const orbx_frame_view* KF2,
                    const orbx_keypoint* dk1, const uint8_t* dd1, const orbx_keypoint* dk2, const uint8_t* dd2,
                    const float* cam, const orbx_mappoint_view* mp1, const uint8_t* valid1,
                    const orbx_mappoint_view* mp2, const uint8_t* valid2, const float* T1w, const float* T2w,
                    float s12, const float* R12, const float* t12, float th, const int32_t* prior12, int32_t* new12,
                    int* n_found)
{
    const int N1 = KF1->n, N2 = KF2->n;
    // vbAlreadyMatched1/2 (:1300-1313) folded into the query masks
    std::vector<uint8_t> q1(N1), q2(N2);
    std::vector<uint8_t> already2(N2, 0);
    for (int i = 0; i < N1; i++)
        if (prior12[i] >= 0 && prior12[i] < N2) already2[prior12[i]] = 1;
    for (int i = 0; i < N1; i++) q1[i] = valid1[i] && prior12[i] == -2;
    for (int i = 0; i < N2; i++) q2[i] = valid2[i] && !already2[i];
    // sR12 = s12*R12, sR21 = (1.0/s12)*R12.t(), t21 = -sR21*t12 (:1284-1286)
    float R1w[9], t1w[3], R2w[9], t2w[3], sR12[9], sR21[9], t21[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) {
            R1w[3 * r + c] = T1w[4 * r + c];
            R2w[3 * r + c] = T2w[4 * r + c];
        }
        t1w[r] = T1w[4 * r + 3];
        t2w[r] = T2w[4 * r + 3];
    }
    const double inv_s = 1.0 / (double)s12;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            sR12[3 * r + c] = (float)((double)s12 * (double)R12[3 * r + c]);
            sR21[3 * r + c] = (float)(inv_s * (double)R12[3 * c + r]);
        }
    for (int r = 0; r < 3; r++) t21[r] = -(sR21[3 * r] * t12[0] + sR21[3 * r + 1] * t12[1] + sR21[3 * r + 2] * t12[2]);
    ctx_enter(ctx);
    ArrayStage s(ctx);
    const ProjStage o1 = stage_proj(s, KF2, mp1, q1.data());   // KF1 points searched in KF2
    const ProjStage o2 = stage_proj(s, KF1, mp2, q2.data());   // KF2 points searched in KF1
    int r = s.upload();
    if (r != ORBX_OK) return r;
    KfProjArgs a{};
    fill_proj(a, s, o1, KF2, mp1, true);
    if (dk2) {
        a.K.kps = dk2;
        a.K.desc = dd2;
    }
    for (int k = 0; k < 4; k++) a.cam[k] = cam[k];
    std::copy(R1w, R1w + 9, a.Ra);
    std::copy(t1w, t1w + 3, a.ta);
    std::copy(sR21, sR21 + 9, a.Rb);
    std::copy(t21, t21 + 3, a.tb);
    a.two_stage = 1;
    a.mode = 2;
    a.th = th;
    if ((r = launch_proj(ctx, a)) != ORBX_OK) return r;
    KfProjArgs b{};
    fill_proj(b, s, o2, KF1, mp2, true);
    if (dk1) {
        b.K.kps = dk1;
        b.K.desc = dd1;
    }
    for (int k = 0; k < 4; k++) b.cam[k] = cam[k];
    std::copy(R2w, R2w + 9, b.Ra);
    std::copy(t2w, t2w + 3, b.ta);
    std::copy(sR12, sR12 + 9, b.Rb);
    std::copy(t12, t12 + 3, b.tb);
    b.two_stage = 1;
    b.mode = 2;
    b.th = th;
    if ((r = launch_proj(ctx, b)) != ORBX_OK) return r;
    std::vector<int32_t> bi1(N1), bd1(N1), bi2(N2), bd2(N2);
    if ((r = s.get(bi1.data(), o1.bi)) || (r = s.get(bd1.data(), o1.bd)) || (r = s.get(bi2.data(), o2.bi)) ||
        (r = s.get(bd2.data(), o2.bd)))
        return r;
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    // bestDist <= TH_HIGH (:1395, :1480), then the agreement check (:1486-1502)
    int nFound = 0;
    for (int i1 = 0; i1 < N1; i1++) {
        new12[i1] = -1;
        const int idx2 = bd1[i1] <= kTHHigh ? bi1[i1] : -1;
        if (idx2 >= 0 && bd2[idx2] <= kTHHigh && bi2[idx2] == i1) {
            new12[i1] = idx2;
            nFound++;
        }
    }
    *n_found = nFound;
    return ORBX_OK;
}

extern "C" int orbx_search_by_sim3(orbx_ctx* ctx, const orbx_frame_view* KF1, const orbx_frame_view* KF2,
                                   const float* cam, const orbx_mappoint_view* mp1, const uint8_t* valid1,
                                   const orbx_mappoint_view* mp2, const uint8_t* valid2, const float* T1w,
                                   const float* T2w, float s12, const float* R12, const float* t12, float th,
                                   const int32_t* prior12, int32_t* new12, int* n_found)
{
    if (!ctx || !valid_frame_view(KF1) || !valid_frame_view(KF2) || !cam || !valid_mps(mp1, false) || !valid_mps(mp2, false) ||
        mp1->n != KF1->n || mp2->n != KF2->n || (KF1->n && (!valid1 || !prior12 || !new12)) ||
        (KF2->n && !valid2) || !T1w || !T2w || !R12 || !t12 || !n_found)
        return ORBX_ERR_ARG;
    return run_sim3(ctx, KF1, KF2, nullptr, nullptr, nullptr, nullptr, cam, mp1, valid1, mp2, valid2, T1w, T2w, s12,
                    R12, t12, th, prior12, new12, n_found);
}

// LoopClosing::ComputeSim3's SearchBySim3 with both keyframes resident in
// their extraction slots.
extern "C" int orbx_dev_search_by_sim3(orbx_ctx* ctx, int slot1, const float* bounds1, int slot2,
                                       const float* bounds2, const float* cam, const orbx_mappoint_view* mp1,
                                       const uint8_t* valid1, const orbx_mappoint_view* mp2, const uint8_t* valid2,
                                       const float* T1w, const float* T2w, float s12, const float* R12,
                                       const float* t12, float th, const int32_t* prior12, int32_t* new12, int cap,
                                       int* n_found)
{
    if (!ctx || slot1 < 0 || slot1 >= ctx->slots || slot2 < 0 || slot2 >= ctx->slots || ctx->geom_w <= 0 || !cam ||
        !valid_mps(mp1, false) || !valid_mps(mp2, false) || !T1w || !T2w || !R12 || !t12 || !n_found || !new12)
        return ORBX_ERR_ARG;
    for (const float* b : {bounds1, bounds2})
        if (b && !(b[1] > b[0] && b[3] > b[2])) return ORBX_ERR_ARG;
    ctx_enter(ctx);
    std::vector<int32_t> cnt;
    if (const int rc = read_slot_counts(ctx, cnt)) return rc;
    const Geometry& g = ctx->geom;
    const int N1 = slot_count(ctx, cnt[slot1]), N2 = slot_count(ctx, cnt[slot2]);
    if (mp1->n != N1 || mp2->n != N2 || (N1 && (!valid1 || !prior12)) || (N2 && !valid2)) return ORBX_ERR_ARG;
    if (cap < N1) return ORBX_ERR_CAPACITY;
    auto view = [&](int n, const float* b) {
        orbx_frame_view v{};
        v.n = n;
        v.min_x = b ? b[0] : 0.f;
        v.max_x = b ? b[1] : (float)g.w;
        v.min_y = b ? b[2] : 0.f;
        v.max_y = b ? b[3] : (float)g.h;
        v.nlevels = g.nlevels;
        v.scale_factor = g.scale_factor;
        return v;
    };
    const orbx_frame_view K1 = view(N1, bounds1), K2 = view(N2, bounds2);
    const FrameDev S1 = slot_frame_dev(ctx, slot1, nullptr), S2 = slot_frame_dev(ctx, slot2, nullptr);
    return run_sim3(ctx, &K1, &K2, S1.kps, S1.desc, S2.kps, S2.desc, cam, mp1, valid1, mp2, valid2, T1w, T2w, s12, R12,
                    t12, th, prior12, new12, n_found);
}

extern "C" int orbx_distinctive_descriptors(orbx_ctx* ctx, int n_mp, const int32_t* obs_ptr, const uint8_t* desc,
                                            int32_t* best)
{
    if (!ctx || n_mp < 0 || (n_mp > 0 && (!obs_ptr || !best))) return ORBX_ERR_ARG;
    if (n_mp == 0) return ORBX_OK;
    if (obs_ptr[0] < 0) return ORBX_ERR_ARG;
    for (int m = 0; m < n_mp; m++)
        if (obs_ptr[m + 1] < obs_ptr[m] || obs_ptr[m + 1] - obs_ptr[m] >= (1 << 20)) return ORBX_ERR_ARG;
    const size_t rows = (size_t)obs_ptr[n_mp];
    if (rows && !desc) return ORBX_ERR_ARG;
    ctx_enter(ctx);
    ArrayStage s(ctx);
    const Region<int32_t> o_ptr = s.take((size_t)n_mp + 1, obs_ptr);
    const Region<uint8_t> o_d = s.take(rows * 32, desc);
    const Region<int32_t> o_b = s.take<int32_t>(n_mp);
    int r = s.upload();
    if (r != ORBX_OK) return r;
    const int per = kBlock / 64;
    hipLaunchKernelGGL(k_distinctive, dim3((n_mp + per - 1) / per), dim3(kBlock), 0, ctx->stream, s.dev(o_ptr),
                       s.dev(o_d), n_mp, s.dev(o_b));
    ORBX_HIP_CHECK(hipGetLastError());
    if ((r = s.get(best, o_b)) != ORBX_OK) return r;
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return ORBX_OK;
}

// SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) against the keyframe
// T, whose keypoints and descriptors are staged here (kf) or already on the
// device (kf null).  matched: T.n entries, in and out.
static int run_kf_sim3(ArrayStage& s, const KfRegions* kf, FrameDev T, int nlevels, float scale_factor,
                       const float* cam, const orbx_mappoint_view* mps, const uint8_t* mp_skip, const float* Scw, int th,
                       int32_t* matched, int* n_matches)
{
    const MpRegions mp = take_mps(s, mps);
    const Region<uint8_t> o_sk = s.take((size_t)mps->n, mp_skip);
    const Region<int32_t> o_out = s.take((size_t)T.n, matched), o_n = s.take<int32_t>(1);
    const int r = s.upload();
    if (r != ORBX_OK) return r;
    if (kf) {
        T.kps = s.dev(kf->kp);
        T.desc = s.dev(kf->kd);
    }
    SeqProjArgs a{};
    set_seq(a, T, nlevels, scale_factor, cam, Scw, 1, (float)th, 0);
    set_mps(a, s, mp, mps->n);
    a.qskip = s.dev(o_sk);
    return run_proj_seq(s, a, o_out, o_n, matched, n_matches);
}

extern "C" int orbx_search_by_projection_kf_sim3(orbx_ctx* ctx, const orbx_frame_view* KF, const float* cam,
                                                 const orbx_mappoint_view* mps, const uint8_t* mp_skip,
                                                 const float* Scw, int th, int32_t* matched, int* n_matches)
{
    if (!ctx || !valid_frame_view(KF) || !cam || !valid_mps(mps, true) || !Scw || !n_matches ||
        (mps->n && !mp_skip) || (KF->n && !matched))
        return ORBX_ERR_ARG;
    ctx_enter(ctx);
    ArrayStage s(ctx);
    const KfRegions kf = take_kf(s, KF);
    return run_kf_sim3(s, &kf, frame_dev(KF, nullptr, nullptr), KF->nlevels, KF->scale_factor, cam, mps, mp_skip, Scw,
                       th, matched, n_matches);
}

// LoopClosing::ComputeSim3 / CorrectLoop's SearchByProjection(pKF, Scw, ...)
// against a keyframe resident in its extraction slot.
extern "C" int orbx_dev_search_by_projection_kf_sim3(orbx_ctx* ctx, int slot, const float* bounds, const float* cam,
                                                     const orbx_mappoint_view* mps, const uint8_t* mp_skip,
                                                     const float* Scw, int th, int32_t* matched, int cap,
                                                     int* n_matches)
{
    if (!ctx || slot < 0 || slot >= ctx->slots || ctx->geom_w <= 0 || !cam || !valid_mps(mps, true) || !Scw ||
        !n_matches || (mps->n && !mp_skip) || !matched)
        return ORBX_ERR_ARG;
    if (bounds && !(bounds[1] > bounds[0] && bounds[3] > bounds[2])) return ORBX_ERR_ARG;
    ctx_enter(ctx);
    int32_t cnt = 0;
    ORBX_HIP_CHECK(hipMemcpyAsync(&cnt, ctx->out_n + slot, 4, hipMemcpyDeviceToHost, ctx->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const int n = slot_count(ctx, cnt);
    if (cap < n) return ORBX_ERR_CAPACITY;
    ArrayStage s(ctx);
    return run_kf_sim3(s, nullptr, kf_slot_dev(ctx, slot, bounds, n), ctx->geom.nlevels, ctx->geom.scale_factor, cam,
                       mps, mp_skip, Scw, th, matched, n_matches);
}

// SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) of the nK
// keyframe keypoints (their keys staged at qk, or at dev_qkps) in the frame
// T, staged (f) or on the device (f null).
static int run_frame_kf(ArrayStage& s, const KfRegions* f, FrameDev T, int nlevels, float scale_factor,
                        Region<orbx_keypoint> qk, const orbx_keypoint* dev_qkps, int nK, const float* cam,
                        const orbx_mappoint_view* kf_mps, const uint8_t* kf_valid, const uint8_t* f_assigned,
                        const float* Tcw, float th, int orb_dist, int check_ori, int32_t* matches_f, int* n_matches)
{
    const Region<float> o_pos = s.take((size_t)nK * 3, kf_mps->pos), o_mn = s.take((size_t)nK, kf_mps->min_dist);
    const Region<uint8_t> o_qd = s.take((size_t)nK * 32, kf_mps->desc), o_sk = s.take<uint8_t>(nK),
                          o_as = s.take((size_t)T.n, f_assigned);
    // at least one entry, all -1 before the search
    const Region<int32_t> o_out = s.take<int32_t>(std::max(T.n, 1)), o_n = s.take<int32_t>(1);
    std::vector<uint8_t> skip(nK);
    for (int i = 0; i < nK; i++) skip[i] = !kf_valid[i];
    s.later(o_sk, skip.data());
    int r = s.upload();
    if (r == ORBX_OK) r = s.fill(o_out, 0xFF);
    if (r != ORBX_OK) return r;
    if (f) {
        T.kps = s.dev(f->kp);
        T.desc = s.dev(f->kd);
    }
    SeqProjArgs a{};
    set_seq(a, T, nlevels, scale_factor, cam, Tcw, 0, th, 1);
    a.orb_dist = orb_dist;
    a.check_ori = check_ori;
    a.nq = nK;
    a.pos = s.dev(o_pos);
    a.dmin = s.dev(o_mn);
    a.qdesc = s.dev(o_qd);
    a.qskip = s.dev(o_sk);
    a.qkps = dev_qkps ? dev_qkps : s.dev(qk);
    a.assigned = s.dev(o_as);
    return run_proj_seq(s, a, o_out, o_n, matches_f, n_matches);
}

extern "C" int orbx_search_by_projection_frame_kf(orbx_ctx* ctx, const orbx_frame_view* F, const orbx_frame_view* KF,
                                                  const float* cam, const orbx_mappoint_view* kf_mps,
                                                  const uint8_t* kf_valid, const uint8_t* f_assigned,
                                                  const float* Tcw, float th, int orb_dist, int check_ori,
                                                  int32_t* matches_f, int* n_matches)
{
    if (!ctx || !valid_frame_view(F) || !valid_frame_view(KF) || !cam || !valid_mps(kf_mps, false) ||
        kf_mps->n != KF->n || !Tcw || !n_matches || (KF->n && !kf_valid) || (F->n && (!f_assigned || !matches_f)))
        return ORBX_ERR_ARG;
    ctx_enter(ctx);
    ArrayStage s(ctx);
    const KfRegions f = take_kf(s, F);
    const Region<orbx_keypoint> qk = s.take((size_t)KF->n, KF->keys_un);
    return run_frame_kf(s, &f, frame_dev(F, nullptr, nullptr), F->nlevels, F->scale_factor, qk, nullptr, KF->n, cam,
                        kf_mps, kf_valid, f_assigned, Tcw, th, orb_dist, check_ori, matches_f, n_matches);
}

// Tracking::Relocalisation's second search, SearchByProjection(CurrentFrame,
// pKF, sAlreadyFound, th, ORBdist), with the current frame and the candidate
// keyframe both resident in their extraction slots: the frame's keypoints
// and descriptors and the keyframe's keypoints are read in HBM; the
// keyframe's map points and the flags are uploaded.
extern "C" int orbx_dev_search_by_projection_frame_kf(orbx_ctx* ctx, int f_slot, const float* f_bounds, int kf_slot,
                                                      const float* cam, const orbx_mappoint_view* kf_mps,
                                                      const uint8_t* kf_valid, const uint8_t* f_assigned,
                                                      const float* Tcw, float th, int orb_dist, int check_ori,
                                                      int32_t* matches_f, int cap, int* n_matches)
{
    if (!ctx || f_slot < 0 || f_slot >= ctx->slots || kf_slot < 0 || kf_slot >= ctx->slots || ctx->geom_w <= 0 ||
        !cam || !valid_mps(kf_mps, false) || !Tcw || !n_matches || !matches_f || !f_assigned ||
        (kf_mps->n && !kf_valid))
        return ORBX_ERR_ARG;
    if (f_bounds && !(f_bounds[1] > f_bounds[0] && f_bounds[3] > f_bounds[2])) return ORBX_ERR_ARG;
    ctx_enter(ctx);
    std::vector<int32_t> cnt;
    if (const int rc = read_slot_counts(ctx, cnt)) return rc;
    const int nF = slot_count(ctx, cnt[f_slot]), nK = slot_count(ctx, cnt[kf_slot]);
    if (kf_mps->n != nK) return ORBX_ERR_ARG;   // one map-point entry per keyframe keypoint
    if (cap < nF) return ORBX_ERR_CAPACITY;
    ArrayStage s(ctx);
    return run_frame_kf(s, nullptr, kf_slot_dev(ctx, f_slot, f_bounds, nF), ctx->geom.nlevels, ctx->geom.scale_factor,
                        {}, slot_frame_dev(ctx, kf_slot, nullptr).kps, nK, cam, kf_mps, kf_valid, f_assigned, Tcw, th,
                        orb_dist, check_ori, matches_f, n_matches);
}

