// New map points on the device: the second half of
// LocalMapping::CreateNewMapPoints' neighbour loop (src/LocalMapping.cc:
// 283-368) -- per match the parallax gate, the 4x4 linear triangulation, the
// depth gates, the two reprojection gates and the scale-consistency gate --
// and the loop itself: SearchForTriangulation (orbx_bow.hip) followed by the
// triangulation of its matches, neighbour after neighbour, a created point
// marking its KF1 keypoint for the searches of the later neighbours (:375,
// src/ORBmatcher.cc:894-896), without leaving the device.
//
// k_triangulate: a lane per (neighbour, KF1 keypoint).  The gates are the
// reference's float arithmetic operation by operation; where OpenCV 2.4
// accumulates in double (the 3x3 products, dot, norm) the sums are FP64 in
// order.  The null vector of the 4x4 A is the defined
// FP64 solve of the initialisation models at 4x4: one-sided Jacobi on A's
// columns, A and V in the lane's registers (32 doubles), V's column of the
// smallest column norm of A V rounded once to float.
#include <algorithm>
#include <cstring>
#include <vector>

#include "orbx_bow_queue.h"
#include "orbx_device.h"
#include "orbx_internal.h"
#include "orbx_jacobi.h"
#include "orbx_linalg.h"
#include "orbx_stage.h"

namespace orbx {

// A keyframe as CreateNewMapPoints reads it (orbx_kf_geom by value).
struct TriGeom {
    float Rcw[9], tcw[3], Ow[3], cam[4];
    float sf[kMaxLevels], sigma2[kMaxLevels];
    int32_t nlevels;
};

// One neighbour of a call.
struct TriJob {
    const orbx_keypoint* k1;
    const orbx_keypoint* k2;
    const int32_t* m12;     // [len] KF2 index per KF1 keypoint, or < 0
    uint8_t* status;        // [len]
    float* xyz;             // [len][3]
    float* v4;              // [len][4]
    int32_t* n_created;
    uint8_t* mark;          // KF1's map-point states: 1 stored where a point was created (null: no marking)
    int32_t n1, n2, len;    // keypoints of KF1 / KF2; entries of the outputs (>= n1, status 0 past n1)
    TriGeom g1, g2;
};

// Rcw.row(r).dot(x3Dt) + tcw(r): cv::Mat::dot sums in double, the float
// translation is added to that double, the assignment rounds (:322, :332).
__device__ inline float cam_coord(const TriGeom& g, int r, const float* x)
{
    return affine3(g.Rcw + 3 * r, x, g.tcw[r]);
}

// The reprojection gate of one keyframe (:331-340, :343-352): true = rejected.
__device__ inline bool reproj_rejects(const TriGeom& g, const orbx_keypoint& kp, const float* x3D, float z, int contract)
{
    const float e2 = reproj_e2(g.cam, cam_coord(g, 0, x3D), cam_coord(g, 1, x3D), z, kp.x, kp.y, contract);
    return (double)e2 > 5.991 * (double)g.sigma2[kp.octave];
}

// One match through the gates in the reference's order: the status of
// orbx.h's table; x3D written for status 1, v4 wherever the solve ran
// (solved).
__device__ inline int triangulate_match(const TriGeom& g1, const TriGeom& g2, const orbx_keypoint& kp1,
                                        const orbx_keypoint& kp2, int contract, float* x3D, float* v4, bool& solved)
{
    solved = false;
    const float invfx1 = 1.0f / g1.cam[0], invfy1 = 1.0f / g1.cam[1];
    const float invfx2 = 1.0f / g2.cam[0], invfy2 = 1.0f / g2.cam[1];
    const float xn1[3] = {(kp1.x - g1.cam[2]) * invfx1, (kp1.y - g1.cam[3]) * invfy1, 1.0f};
    const float xn2[3] = {(kp2.x - g2.cam[2]) * invfx2, (kp2.y - g2.cam[3]) * invfy2, 1.0f};
    float ray1[3], ray2[3];
    tmatvec3(g1.Rcw, xn1, ray1);   // ray = Rwc * xn (:294)
    tmatvec3(g2.Rcw, xn2, ray2);
    // the quotient by the double product of the norms (reconstruction divides by the float product)
    const float cosv = (float)(dot3(ray1, ray2) / (norm3(ray1) * norm3(ray2)));
    if (cosv < 0.f || (double)cosv > 0.9998) return 2;

    // A.row(0) = xn1(0) * Tcw1.row(2) - Tcw1.row(0), ... (:303-307)
    float A[16];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float t10 = j < 3 ? g1.Rcw[j] : g1.tcw[0], t11 = j < 3 ? g1.Rcw[3 + j] : g1.tcw[1],
                    t12 = j < 3 ? g1.Rcw[6 + j] : g1.tcw[2];
        const float t20 = j < 3 ? g2.Rcw[j] : g2.tcw[0], t21 = j < 3 ? g2.Rcw[3 + j] : g2.tcw[1],
                    t22 = j < 3 ? g2.Rcw[6 + j] : g2.tcw[2];
        A[j] = xn1[0] * t12 - t10;
        A[4 + j] = xn1[1] * t12 - t11;
        A[8 + j] = xn2[0] * t22 - t20;
        A[12 + j] = xn2[1] * t22 - t21;
    }
    null_vector4(A, v4);
    solved = true;
    if (v4[3] == 0.f) return 3;
    // x3D.rowRange(0,3) / x3D(3): a scaled convert, the float scale 1 / x3D(3)
    const float inv = (float)(1.0 / (double)v4[3]);
    const float x[3] = {v4[0] * inv, v4[1] * inv, v4[2] * inv};

    const float z1 = cam_coord(g1, 2, x);
    if (z1 <= 0.f) return 4;
    const float z2 = cam_coord(g2, 2, x);
    if (z2 <= 0.f) return 5;
    if (reproj_rejects(g1, kp1, x, z1, contract)) return 6;
    if (reproj_rejects(g2, kp2, x, z2, contract)) return 7;

    const float nrm1[3] = {x[0] - g1.Ow[0], x[1] - g1.Ow[1], x[2] - g1.Ow[2]};
    const float nrm2[3] = {x[0] - g2.Ow[0], x[1] - g2.Ow[1], x[2] - g2.Ow[2]};
    const float dist1 = (float)norm3(nrm1);
    const float dist2 = (float)norm3(nrm2);
    if (dist1 == 0.f || dist2 == 0.f) return 8;
    const float ratioDist = dist1 / dist2;
    const float ratioOctave = g1.sf[kp1.octave] / g2.sf[kp2.octave];
    const float ratioFactor = 1.5f * g1.sf[1];
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return 9;
    x3D[0] = x[0];
    x3D[1] = x[1];
    x3D[2] = x[2];
    return 1;
}

__global__ __launch_bounds__(256) void k_triangulate(const TriJob* __restrict__ jobs, int contract)
{
    const TriJob& j = jobs[blockIdx.y];
    const int i1 = blockIdx.x * blockDim.x + threadIdx.x;
    if (i1 >= j.len) return;
    int st = 0;
    if (i1 < j.n1) {
        const int i2 = j.m12[i1];
        if (i2 >= 0 && i2 < j.n2) {
            const orbx_keypoint kp1 = j.k1[i1];
            const orbx_keypoint kp2 = j.k2[i2];
            // an octave outside the level tables is no match (the host forms reject it before the launch)
            if (kp1.octave >= 0 && kp1.octave < j.g1.nlevels && kp2.octave >= 0 && kp2.octave < j.g2.nlevels) {
                float x3D[3], v4[4];
                bool solved;
                st = triangulate_match(j.g1, j.g2, kp1, kp2, contract, x3D, v4, solved);
                if (solved) {
#pragma unroll
                    for (int c = 0; c < 4; c++) j.v4[4 * (size_t)i1 + c] = v4[c];
                }
                if (st == 1) {
#pragma unroll
                    for (int c = 0; c < 3; c++) j.xyz[3 * (size_t)i1 + c] = x3D[c];
                    if (j.mark) j.mark[i1] = 1;
                    atomicAdd(j.n_created, 1);
                }
            }
        }
    }
    j.status[i1] = (uint8_t)st;
}

namespace {

// Argument rules of one orbx_kf_geom (before any device work).
bool valid_geom(const orbx_kf_geom* g)
{
    return g && g->Rcw && g->tcw && g->Ow && g->cam && g->scale_factors && g->level_sigma2 && g->nlevels >= 2 &&
           g->nlevels <= kMaxLevels;
}

TriGeom to_dev(const orbx_kf_geom& g)
{
    TriGeom t{};
    std::memcpy(t.Rcw, g.Rcw, sizeof(t.Rcw));
    std::memcpy(t.tcw, g.tcw, sizeof(t.tcw));
    std::memcpy(t.Ow, g.Ow, sizeof(t.Ow));
    std::memcpy(t.cam, g.cam, sizeof(t.cam));
    for (int l = 0; l < g.nlevels; l++) {
        t.sf[l] = g.scale_factors[l];
        t.sigma2[l] = g.level_sigma2[l];
    }
    t.nlevels = g.nlevels;
    return t;
}

// One neighbour's result block: status | xyz | v4 | n_created.
struct TriLayout {
    size_t o_xyz, o_v4, o_n, stride;
    int len;
};

TriLayout tri_layout(int len)
{
    TriLayout L;
    BlockOffsets o;
    L.len = len;
    o.take(len);   // status
    L.o_xyz = o.take((long long)len * 12);
    L.o_v4 = o.take((long long)len * 16);
    L.o_n = o.take(16);
    L.stride = o.end;
    return L;
}

void point_job(TriJob& j, uint8_t* res, const TriLayout& L)
{
    j.status = res;
    j.xyz = reinterpret_cast<float*>(res + L.o_xyz);
    j.v4 = reinterpret_cast<float*>(res + L.o_v4);
    j.n_created = reinterpret_cast<int32_t*>(res + L.o_n);
    j.len = L.len;
}

int launch_triangulate(orbx_ctx* ctx, const TriJob* jobs, int n, int len)
{
    if (n <= 0 || len <= 0) return ORBX_OK;
    timer_begin(ctx, "triangulate");
    hipLaunchKernelGGL(k_triangulate, dim3((len + 255) / 256, n), dim3(256), 0, ctx->stream, jobs, ctx->fp_contract);
    timer_end(ctx, "triangulate");
    ORBX_HIP_CHECK(hipGetLastError());
    return ORBX_OK;
}

// The result blocks (host copy) into the caller's arrays: status whole, xyz
// where a point was created, the v4 tap where the solve ran.
void scatter_results(const ResultBlocks& res, const TriLayout& L, int n, float* const* xyz, uint8_t* const* status,
                     int* n_created, float* const* v4)
{
    for (int k = 0; k < n; k++) {
        const uint8_t* blk = res.block(k);
        const float* x = reinterpret_cast<const float*>(blk + L.o_xyz);
        const float* v = reinterpret_cast<const float*>(blk + L.o_v4);
        if (L.len) std::memcpy(status[k], blk, L.len);
        for (int i = 0; i < L.len; i++) {
            const int st = blk[i];
            if (st == 1) std::memcpy(xyz[k] + 3 * (size_t)i, x + 3 * (size_t)i, 12);
            if (v4 && v4[k] && st != 0 && st != 2) std::memcpy(v4[k] + 4 * (size_t)i, v + 4 * (size_t)i, 16);
        }
        std::memcpy(&n_created[k], blk + L.o_n, 4);
    }
}

}  // namespace
}  // namespace orbx

using namespace orbx;

extern "C" int orbx_triangulate_matches(orbx_ctx* ctx, const orbx_keypoint* keys1, int n1, const orbx_kf_geom* g1, int n,
                                        const orbx_keypoint* const* keys2, const int* n2s, const orbx_kf_geom* g2s,
                                        const int32_t* const* matches12, float* const* xyz, uint8_t* const* status,
                                        int* n_created, float* const* v4)
{
    if (!ctx || n < 0 || n1 < 0) return ORBX_ERR_ARG;
    if (n == 0 || n1 == 0) return ORBX_OK;
    if (!keys1 || !valid_geom(g1) || !keys2 || !n2s || !g2s || !matches12 || !xyz || !status || !n_created)
        return ORBX_ERR_ARG;
    if (n1 > kMaxFeatures) return ORBX_ERR_UNSUPPORTED;
    if (!octaves_ok(keys1, n1, g1->nlevels)) return ORBX_ERR_ARG;
    // one upload: jobs | keypoints (KF1, then each KF2) | matches; then the result blocks
    PackedStage st(ctx);
    const Region<TriJob> jobs = st.take<TriJob>(n);
    const Region<orbx_keypoint> kps1 = st.take(n1, keys1);
    std::vector<Region<orbx_keypoint>> kps2(n);
    for (int k = 0; k < n; k++) {
        if (n2s[k] < 0 || !valid_geom(&g2s[k]) || !matches12[k] || !xyz[k] || !status[k] || (n2s[k] > 0 && !keys2[k]))
            return ORBX_ERR_ARG;
        if (n2s[k] > kMaxFeatures) return ORBX_ERR_UNSUPPORTED;
        if (!octaves_ok(keys2[k], n2s[k], g2s[k].nlevels)) return ORBX_ERR_ARG;
        for (int i = 0; i < n1; i++)
            if (matches12[k][i] >= n2s[k]) return ORBX_ERR_ARG;   // the reference would index past KF2's keypoints
        kps2[k] = st.take(n2s[k], keys2[k]);
    }
    std::vector<Region<int32_t>> m12(n);
    for (int k = 0; k < n; k++) m12[k] = st.take(n1, matches12[k]);
    ctx_enter(ctx);
    const TriLayout L = tri_layout(n1);
    int r = st.open((size_t)n * L.stride);
    if (r != ORBX_OK) return r;
    ResultBlocks res(ctx, st.behind(), n, L.stride);
    const TriGeom G1 = to_dev(*g1);
    for (int k = 0; k < n; k++) {
        TriJob& j = st.host(jobs)[k];
        j.k1 = st.dev(kps1);
        j.k2 = st.dev(kps2[k]);
        j.m12 = st.dev(m12[k]);
        j.mark = nullptr;
        j.n1 = n1;
        j.n2 = n2s[k];
        j.g1 = G1;
        j.g2 = to_dev(g2s[k]);
        point_job(j, res.dev + (size_t)k * L.stride, L);
    }
    if ((r = st.upload()) != ORBX_OK || (r = res.zero()) != ORBX_OK) return r;
    if ((r = launch_triangulate(ctx, st.dev(jobs), n, n1)) != ORBX_OK) return r;
    if ((r = res.read()) != ORBX_OK) return r;
    scatter_results(res, L, n, xyz, status, n_created, v4);
    return ORBX_OK;
}

namespace {

// The part the two loop forms share: the searches are queued by `queue`
// (orbx_bow_queue.h; with a callback when chained), the triangulation jobs
// are built from what it left on the device, and everything is read back
// after one synchronisation.
struct NewPointsCall {
    orbx_ctx* ctx;
    int n, chain;
    const orbx_kf_geom* g1;
    const orbx_kf_geom* g2s;
    BowQueued q;
    TriLayout L{};
    PackedStage st{ctx};   // the jobs, ahead of the result blocks, in the search's extra bytes
    Region<TriJob> jobs = st.take<TriJob>(n);
    bool prepared = false;

    size_t extra_bytes(int len) const { return st.total + (size_t)n * tri_layout(len).stride; }
    TriJob* dev_jobs() const { return st.dev(jobs); }
    uint8_t* dev_res() const { return st.behind(); }

    // jobs uploaded, result blocks zeroed (once q is filled)
    int prepare()
    {
        if (prepared) return ORBX_OK;
        prepared = true;
        L = tri_layout(q.out_len);
        st.bind(q.extra);
        const TriGeom G1 = to_dev(*g1);
        for (int k = 0; k < n; k++) {
            TriJob& j = st.host(jobs)[k];
            j.k1 = q.k1;
            j.k2 = q.k2[k];
            j.m12 = q.out[k];
            j.mark = chain ? q.mp1 : nullptr;
            j.n1 = q.n1;
            j.n2 = q.n2[k];
            j.g1 = G1;
            j.g2 = to_dev(g2s[k]);
            point_job(j, dev_res() + (size_t)k * L.stride, L);
        }
        const int r = st.upload();
        return r != ORBX_OK ? r : ResultBlocks(ctx, dev_res(), n, L.stride).zero();
    }

    int after(int k)
    {
        int r = prepare();
        if (r != ORBX_OK) return r;
        return launch_triangulate(ctx, dev_jobs() + k, 1, L.len);
    }

    // chain 0: the one launch over all neighbours; then the read-back
    int finish(int32_t* const* matches12, int* n_matches, float* const* xyz, uint8_t* const* status, int* n_created,
               float* const* v4)
    {
        int r;
        if (!chain) {
            if ((r = prepare()) != ORBX_OK) return r;
            if ((r = launch_triangulate(ctx, dev_jobs(), n, L.len)) != ORBX_OK) return r;
        }
        if ((r = read_bow_queued(ctx, q, q.out_len, matches12, n_matches)) != ORBX_OK) return r;
        ResultBlocks res(ctx, dev_res(), n, L.stride);
        if ((r = res.read()) != ORBX_OK) return r;
        scatter_results(res, L, n, xyz, status, n_created, v4);
        return ORBX_OK;
    }
};

bool outputs_ok(int n, int32_t* const* matches12, const int* n_matches, float* const* xyz, uint8_t* const* status,
                const int* n_created)
{
    if (!matches12 || !n_matches || !xyz || !status || !n_created) return false;
    for (int k = 0; k < n; k++)
        if (!matches12[k] || !xyz[k] || !status[k]) return false;
    return true;
}

}  // namespace

extern "C" int orbx_create_new_map_points(orbx_ctx* ctx, const orbx_bow_view* KF1, const orbx_kf_geom* g1, int n,
                                          const orbx_bow_view* KF2s, const orbx_kf_geom* g2s, const float* F12s,
                                          int check_ori, int chain, int32_t* const* matches12, int* n_matches,
                                          float* const* xyz, uint8_t* const* status, int* n_created, float* const* v4)
{
    if (!ctx || !KF1 || n < 0 || KF1->n < 0) return ORBX_ERR_ARG;
    if (n == 0 || KF1->n == 0) return ORBX_OK;
    if (!valid_geom(g1) || !KF2s || !g2s || !F12s || !KF1->keys || !outputs_ok(n, matches12, n_matches, xyz, status, n_created))
        return ORBX_ERR_ARG;
    if (!octaves_ok(KF1->keys, KF1->n, g1->nlevels)) return ORBX_ERR_ARG;
    int nl = 0;
    for (int k = 0; k < n; k++) {
        if (!valid_geom(&g2s[k]) || KF2s[k].n < 0 || (KF2s[k].n > 0 && !KF2s[k].keys)) return ORBX_ERR_ARG;
        if (!octaves_ok(KF2s[k].keys, KF2s[k].n, g2s[k].nlevels)) return ORBX_ERR_ARG;
        nl = std::max(nl, g2s[k].nlevels);
        if (chain)   // a created point changes KF2's states too: one KF2 per chained call
            for (int m = 0; m < k; m++)
                if ((KF2s[k].keys && KF2s[k].keys == KF2s[m].keys) || (KF2s[k].mp && KF2s[k].mp == KF2s[m].mp))
                    return ORBX_ERR_ARG;
    }
    // the searches read KF2's mvLevelSigma2 at a common stride
    std::vector<float> sigma2s((size_t)n * nl, 0.f);
    for (int k = 0; k < n; k++) std::copy(g2s[k].level_sigma2, g2s[k].level_sigma2 + g2s[k].nlevels, sigma2s.begin() + (size_t)k * nl);
    NewPointsCall c{ctx, n, chain != 0, g1, g2s};
    const BowAfter after = [&](int k) { return c.after(k); };
    int r = queue_bow_batch(ctx, KF1, n, KF2s, 2, 0.f, check_ori, F12s, sigma2s.data(), nl, c.extra_bytes(KF1->n),
                            chain ? &after : nullptr, &c.q);
    if (r != ORBX_OK) return r;
    return c.finish(matches12, n_matches, xyz, status, n_created, v4);
}

extern "C" int orbx_dev_create_new_map_points(orbx_ctx* ctx, int slot1, const uint8_t* mp1, const orbx_kf_geom* g1, int n,
                                              const int* slots2, const uint8_t* const* mp2s, const orbx_kf_geom* g2s,
                                              const float* F12s, int check_ori, int chain, int32_t* const* matches12,
                                              int* n_matches, float* const* xyz, uint8_t* const* status,
                                              int* n_created, float* const* v4, int cap)
{
    if (!ctx || n < 0) return ORBX_ERR_ARG;
    if (n == 0) return ORBX_OK;
    if (!mp1 || !valid_geom(g1) || !slots2 || !mp2s || !g2s || !F12s ||
        !outputs_ok(n, matches12, n_matches, xyz, status, n_created))
        return ORBX_ERR_ARG;
    const int nl = ctx->geom.nlevels;   // octaves index the level tables
    if (g1->nlevels != nl) return ORBX_ERR_ARG;
    for (int k = 0; k < n; k++) {
        if (!valid_geom(&g2s[k]) || g2s[k].nlevels != nl) return ORBX_ERR_ARG;
        if (chain)
            for (int m = 0; m < k; m++)
                if (slots2[k] == slots2[m]) return ORBX_ERR_ARG;
    }
    std::vector<float> sigma2s((size_t)n * nl);
    for (int k = 0; k < n; k++) std::copy(g2s[k].level_sigma2, g2s[k].level_sigma2 + nl, sigma2s.begin() + (size_t)k * nl);
    NewPointsCall c{ctx, n, chain != 0, g1, g2s};
    const BowAfter after = [&](int k) { return c.after(k); };
    int r = queue_bow_slots(ctx, 2, slot1, mp1, n, slots2, mp2s, 0.f, check_ori, F12s, sigma2s.data(), nl, cap,
                            c.extra_bytes(std::max(ctx->bow_nf, 1)), chain ? &after : nullptr, &c.q);
    if (r != ORBX_OK) return r;
    if ((r = c.finish(matches12, n_matches, xyz, status, n_created, v4)) != ORBX_OK) return r;
    for (int k = 0; k < n; k++)
        if (n_matches[k] < 0) return ORBX_ERR_UNSUPPORTED;
    return ORBX_OK;
}
