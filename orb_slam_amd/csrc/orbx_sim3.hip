// Sim3Solver on the device (src/Sim3Solver.cc): the constructor, and one
// Sim3Solver::iterate call with every RANSAC iteration of the call evaluated
// at once from the caller's rand() draws.
//
// Three kernels per call, each over all candidate pairs of the call:
//   k_sim3_prepare  a workgroup per pair: wave 0 walks i1 in order, keeps the
//                   correspondences (ballot prefix) and computes for each the
//                   camera coordinates, their projections and the integer
//                   error limits; then a thread per iteration draws its
//                   minimal set (vAvailableIndices as a list of overwritten
//                   places in registers).
//   k_sim3_solve    computeT, a lane per hypothesis, everything in registers:
//                   centroids, M, N, a two-sided FP64 Jacobi on the symmetric
//                   4x4 N (eigenvalues with their signs), Rodrigues, scale,
//                   translation, T12 and T21.
//   k_sim3_check    a workgroup per pair: the correspondences staged in LDS
//                   (tiles of 1024), a lane per (iteration, slice of the
//                   correspondences), integer counts summed with LDS atomics;
//                   then thread 0 replays iterate's sequential bookkeeping
//                   over the counts and the workgroup recomputes the inlier
//                   mask of the returned iteration.
//
// The reference's own float expressions are followed operation by operation;
// the places that go through OpenCV are the definitions of DESIGN.md
// section 4 (tests/sim3_numpy.py restates all of it).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "orbx_bow_queue.h"
#include "orbx_device.h"
#include "orbx_internal.h"
#include "orbx_jacobi.h"
#include "orbx_linalg.h"
#include "orbx_stage.h"

namespace orbx {

constexpr int kSim3MaxIter = 1024;
constexpr int kSim3Tile = 1024;    // correspondences staged per LDS tile
constexpr int kSim3Floats = 12;    // per staged correspondence

struct Sim3Hdr {
    int32_t N, max_its, iters_run, no_more;
    int32_t found, found_iter, n_inliers, best_out;
    int32_t best_iter, discarded, run, pad;
    float T12[16];
    float R12[9], t12[3], s12;
    float pad1[3];
};

// One candidate pair: device pointers to its inputs and the solver's state.
struct Sim3Pair {
    const orbx_keypoint* k1;
    const orbx_keypoint* k2;
    const int32_t* m12;
    const int32_t* idx1;       // or null
    const float* pos1;
    const float* pos2;
    const uint8_t* valid1;     // 1 = a good map point
    const uint8_t* valid2;
    const float* sigma2_1;
    const float* sigma2_2;
    const int32_t* draws;
    const int32_t* its_table;  // mRansacMaxIts by N (used when max_its < 0)
    const int32_t* n_matches;  // the search's count (device-resident form), or null
    int32_t n1, n2, nlevels;
    int32_t min_inliers, max_its, min_matches;
    int32_t iter_done, best_in, n_iter;
    float T1w[12], T2w[12];    // rows 0..2 of Tcw
    float cam1[4], cam2[4];
};

// Byte offsets inside one pair's result block.
struct Sim3Layout {
    long long stride;
    int o_idx, o_x1, o_x2, o_p1, o_p2, o_l1, o_l2, o_sets, o_q, o_R, o_s, o_T12, o_T21, o_cnt, o_inl;
    int M, cap;
};

inline Sim3Layout sim3_layout(int M, int cap)
{
    Sim3Layout L;
    BlockOffsets o;
    o.take(sizeof(Sim3Hdr));
    L.o_idx = o.take((long long)cap * 4);
    L.o_x1 = o.take((long long)cap * 12);
    L.o_x2 = o.take((long long)cap * 12);
    L.o_p1 = o.take((long long)cap * 8);
    L.o_p2 = o.take((long long)cap * 8);
    L.o_l1 = o.take((long long)cap * 4);
    L.o_l2 = o.take((long long)cap * 4);
    L.o_sets = o.take((long long)M * 12);
    L.o_q = o.take((long long)M * 16);
    L.o_R = o.take((long long)M * 36);
    L.o_s = o.take((long long)M * 4);
    L.o_T12 = o.take((long long)M * 64);
    L.o_T21 = o.take((long long)M * 64);
    L.o_cnt = o.take((long long)M * 4);
    L.o_inl = o.take(cap);
    L.stride = o.end;
    L.M = M;
    L.cap = cap;
    return L;
}

// fx*x+cx (:396, :416), the reference's own source: follows orbx_set_fp_contract
__device__ inline float to_pixel(float f, float x, float c, int contract) { return contract ? fmaf(f, x, c) : f * x + c; }

// FromCameraToImage / Project's tail (:392-396, :412-416).  Not reproj_e2's
// projection: the divide is in float, and x meets 1/z before f.
__device__ inline void cam_to_image(const float* cam, float X, float Y, float Z, int contract, float& u, float& v)
{
    const float invz = 1.f / Z;
    const float x = X * invz;
    const float y = Y * invz;
    u = to_pixel(cam[0], x, cam[2], contract);
    v = to_pixel(cam[1], y, cam[3], contract);
}

// ---------------------------------------------------------------------------
// k_sim3_prepare
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sim3_prepare(const Sim3Pair* __restrict__ descs, uint8_t* __restrict__ res,
                                                      Sim3Layout L, int contract)
{
    __shared__ int s_n;
    const Sim3Pair& d = descs[blockIdx.x];
    uint8_t* blk = res + (long long)blockIdx.x * L.stride;
    Sim3Hdr* hdr = reinterpret_cast<Sim3Hdr*>(blk);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n1 = max(0, min(d.n1, L.cap));
    const int n2 = max(0, d.n2);
    const bool discarded = d.n_matches && *d.n_matches < d.min_matches;

    if (wave == 0) {
        int32_t* indices1 = reinterpret_cast<int32_t*>(blk + L.o_idx);
        float* x1 = reinterpret_cast<float*>(blk + L.o_x1);
        float* x2 = reinterpret_cast<float*>(blk + L.o_x2);
        float* p1 = reinterpret_cast<float*>(blk + L.o_p1);
        float* p2 = reinterpret_cast<float*>(blk + L.o_p2);
        int32_t* l1 = reinterpret_cast<int32_t*>(blk + L.o_l1);
        int32_t* l2 = reinterpret_cast<int32_t*>(blk + L.o_l2);
        const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
        int base = 0;
        for (int c = 0; c < n1 && !discarded; c += 64) {
            const int i1 = c + lane;
            int ka = -1, kb = -1, oa = 0, ob = 0;
            bool ok = false;
            if (i1 < n1) {
                kb = d.m12[i1];
                ka = d.idx1 ? d.idx1[i1] : i1;
                ok = kb >= 0 && kb < n2 && ka >= 0 && ka < n1;
                if (ok) ok = d.valid1[ka] == 1 && d.valid2[kb] == 1;
                if (ok) {
                    oa = d.k1[ka].octave;
                    ob = d.k2[kb].octave;
                    ok = oa >= 0 && oa < d.nlevels && ob >= 0 && ob < d.nlevels;
                }
            }
            const unsigned long long bal = __ballot(ok);
            if (ok) {
                const int pos = base + __popcll(bal & lt_mask);   // < n1 <= cap
                indices1[pos] = i1;
                // mvnMaxError (:87-88): a double product truncated into a size_t
                l1[pos] = (int32_t)(9.210 * (double)d.sigma2_1[oa]);
                l2[pos] = (int32_t)(9.210 * (double)d.sigma2_2[ob]);
                // Rcw*X3Dw+tcw (:95, :98)
                const float* a = d.pos1 + 3 * ka;
                const float* b = d.pos2 + 3 * kb;
                float ca[3], cb[3];
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    ca[r] = affine3(d.T1w + 4 * r, a, d.T1w[4 * r + 3]);
                    cb[r] = affine3(d.T2w + 4 * r, b, d.T2w[4 * r + 3]);
                    x1[3 * pos + r] = ca[r];
                    x2[3 * pos + r] = cb[r];
                }
                float u, v;
                cam_to_image(d.cam1, ca[0], ca[1], ca[2], contract, u, v);
                p1[2 * pos] = u;
                p1[2 * pos + 1] = v;
                cam_to_image(d.cam2, cb[0], cb[1], cb[2], contract, u, v);
                p2[2 * pos] = u;
                p2[2 * pos + 1] = v;
            }
            base += __popcll(bal);
        }
        if (lane == 0) s_n = base;
    }
    __syncthreads();
    const int N = s_n;
    const bool run = !discarded && N >= d.min_inliers && N >= 3;
    if (tid == 0) {
        hdr->N = N;
        hdr->max_its = d.max_its >= 0 ? d.max_its : d.its_table[min(N, kMaxFeatures)];
        hdr->discarded = discarded;
        hdr->run = run;
    }
    if (!run) return;   // the block was cleared: sets and the later taps read zero
    // the minimal sets (:163-177): vAvailableIndices is the identity but for
    // the places earlier picks of this iteration overwrote, kept as a list.
    // The removal writes at the drawn *value* (:175), so pos[] holds values.
    int32_t* sets = reinterpret_cast<int32_t*>(blk + L.o_sets);
    const int M = min(d.n_iter, L.M);
    for (int it = tid; it < M; it += blockDim.x) {
        int pos[3], val[3];
        const int32_t* dr = d.draws + (long long)it * 3;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int size = N - j;
            const int randi = (int)(((double)dr[j] / 2147483648.0) * (double)size);
            int idx = randi;
            int back = size - 1;
#pragma unroll
            for (int k = 0; k < 3; k++)
                if (k < j) {
                    if (pos[k] == randi) idx = val[k];
                    if (pos[k] == size - 1) back = val[k];
                }
            pos[j] = idx;
            val[j] = back;
            sets[it * 3 + j] = idx;
        }
    }
}

// ---------------------------------------------------------------------------
// k_sim3_solve
// ---------------------------------------------------------------------------
// The unit eigenvector of the symmetric 4x4 N (float entries n[10]: N11 N12
// N13 N14 N22 N23 N24 N33 N34 N44) for its largest eigenvalue: a two-sided
// cyclic Jacobi in FP64 (the diagonal ends as the eigenvalues with their
// signs; N is traceless, so the largest is in general not the one of largest
// magnitude), rounded once to float, with q0 >= 0.  A NaN entry rotates
// nothing and gives NaNs.
__device__ inline void top_eigenvector4(const float* n, float* q)
{
    double a[4][4], v[4][4];   // a symmetric; v[column][row]
    a[0][0] = (double)n[0];
    a[0][1] = a[1][0] = (double)n[1];
    a[0][2] = a[2][0] = (double)n[2];
    a[0][3] = a[3][0] = (double)n[3];
    a[1][1] = (double)n[4];
    a[1][2] = a[2][1] = (double)n[5];
    a[1][3] = a[3][1] = (double)n[6];
    a[2][2] = (double)n[7];
    a[2][3] = a[3][2] = (double)n[8];
    a[3][3] = (double)n[9];
    double frob = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            v[i][j] = i == j ? 1.0 : 0.0;
            frob += a[i][j] * a[i][j];
        }
    const double floor = (kInitTol * kInitTol) * frob;   // off-diagonals below 4 eps |N|_F are left
    for (int sweep = 0; sweep < kInitSweeps; sweep++) {
        bool rot = false;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int r = p + 1; r < 4; r++) {
                const double apq = a[p][r];
                if (sym_wants(apq, floor)) {
                    rot = true;
                    const JacobiRot g = jacobi_cs(a[p][p], a[r][r], apq);
                    const double c = g.c, s = g.s, t = g.t;
                    a[p][p] = a[p][p] - t * apq;
                    a[r][r] = a[r][r] + t * apq;
                    a[p][r] = a[r][p] = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (k != p && k != r) {
                            const double akp = a[k][p], akq = a[k][r];
                            a[k][p] = a[p][k] = c * akp - s * akq;
                            a[k][r] = a[r][k] = s * akp + c * akq;
                        }
                        const double vp = v[p][k], vq = v[r][k];
                        v[p][k] = c * vp - s * vq;
                        v[r][k] = s * vp + c * vq;
                    }
                }
            }
        if (!rot) break;
    }
    int best = 0;
    double top = a[0][0];
#pragma unroll
    for (int j = 1; j < 4; j++)
        if (a[j][j] > top) {
            top = a[j][j];
            best = j;
        }
    double e[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        e[k] = v[0][k];
#pragma unroll
        for (int j = 1; j < 4; j++)
            if (best == j) e[k] = v[j][k];
    }
    // q and -q are one rotation but not the same bits downstream: q0 >= 0
    // (a zero q0: the first non-zero of the rest positive)
    bool neg = e[0] < 0.0;
    if (e[0] == 0.0) neg = e[1] < 0.0 || (e[1] == 0.0 && (e[2] < 0.0 || (e[2] == 0.0 && e[3] < 0.0)));
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = (float)(neg ? -e[k] : e[k]);
}

__global__ __launch_bounds__(64) void k_sim3_solve(const Sim3Pair* __restrict__ descs, uint8_t* __restrict__ res,
                                                   Sim3Layout L)
{
    const Sim3Pair& d = descs[blockIdx.y];
    uint8_t* blk = res + (long long)blockIdx.y * L.stride;
    const Sim3Hdr* hdr = reinterpret_cast<const Sim3Hdr*>(blk);
    const int M = min(d.n_iter, L.M);
    const int it = blockIdx.x * blockDim.x + threadIdx.x;
    if (!hdr->run || it >= M) return;
    const int N = hdr->N;
    const int32_t* set = reinterpret_cast<const int32_t*>(blk + L.o_sets) + it * 3;
    const float* x1 = reinterpret_cast<const float*>(blk + L.o_x1);
    const float* x2 = reinterpret_cast<const float*>(blk + L.o_x2);

    // P3Dc1i / P3Dc2i (:172-173): column j is the set's j-th correspondence
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int idx = min(max(set[j], 0), N - 1);
#pragma unroll
        for (int r = 0; r < 3; r++) {
            P1[r][j] = x1[3 * idx + r];
            P2[r][j] = x2[3 * idx + r];
        }
    }
    // centroid (:215-224): cv::reduce sums a row in float, C/P.cols scales by float(1.0/3)
    const float third = (float)(1.0 / 3.0);
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        float s1 = P1[r][0] + P1[r][1];
        s1 = s1 + P1[r][2];
        float s2 = P2[r][0] + P2[r][1];
        s2 = s2 + P2[r][2];
        O1[r] = s1 * third;
        O2[r] = s2 * third;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            Pr1[r][j] = P1[r][j] - O1[r];
            Pr2[r][j] = P2[r][j] - O2[r];
        }
    }
    // M = Pr2*Pr1.t() (:243)
    float Mm[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Mm[i][j] = (float)dot3(Pr2[i], Pr1[j]);
    // N (:251-265): sums and differences of floats are float arithmetic
    float n[10];
    n[0] = Mm[0][0] + Mm[1][1] + Mm[2][2];
    n[1] = Mm[1][2] - Mm[2][1];
    n[2] = Mm[2][0] - Mm[0][2];
    n[3] = Mm[0][1] - Mm[1][0];
    n[4] = Mm[0][0] - Mm[1][1] - Mm[2][2];
    n[5] = Mm[0][1] + Mm[1][0];
    n[6] = Mm[2][0] + Mm[0][2];
    n[7] = -Mm[0][0] + Mm[1][1] - Mm[2][2];
    n[8] = Mm[1][2] + Mm[2][1];
    n[9] = -Mm[0][0] - Mm[1][1] + Mm[2][2];
    float q[4];
    top_eigenvector4(n, q);
    // ang (:278) and the angle-axis vector (:280): a scaled convert with the
    // float scale float((2*ang)*(1/norm))
    const double nrm = norm3(q + 1);
    const double ang = atan2(nrm, (double)q[0]);
    const float av = (float)((2.0 * ang) * (1.0 / nrm));
    const float vec[3] = {q[1] * av, q[2] * av, q[3] * av};
    // cv::Rodrigues (:284), in double from the float vector
    float R[9];
    {
        double rx = (double)vec[0], ry = (double)vec[1], rz = (double)vec[2];
        const double theta = sqrt((rx * rx + ry * ry) + rz * rz);
        if (theta < 2.220446049250313e-16) {
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.f : 0.f;
        } else {
            const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, itheta = 1.0 / theta;
            rx *= itheta;
            ry *= itheta;
            rz *= itheta;
            const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
            const double rcr[9] = {0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0};
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = (float)((c * ((k % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[k]) + s * rcr[k]);
        }
    }
    // P3 = mR12i*Pr2 (:288), nom = Pr1.dot(P3) (:292), den (:295-304): sums
    // of nine terms in the walk's order, so no dot3
    double nom = 0.0, den = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float p3 = (float)dot3(R + 3 * i, Pr2[0][j], Pr2[1][j], Pr2[2][j]);
            nom = nom + (double)Pr1[i][j] * (double)p3;
            den = den + (double)(p3 * p3);
        }
    const float s12 = (float)(nom / den);   // ms12i (:306)
    // mt12i = O1 - ms12i*mR12i*O2 (:311): the gemm with alpha = -s and addend O1
    float t[3];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = (float)(-(double)s12 * dot3(R + 3 * i, O2) + (double)O1[i]);
    // T12 (:316-321), T21 (:325-331)
    const float sinv = (float)(1.0 / (double)s12);
    float T12[16], T21[16], sRinv[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            T12[4 * i + j] = R[3 * i + j] * s12;
            sRinv[3 * i + j] = R[3 * j + i] * sinv;
            T21[4 * i + j] = sRinv[3 * i + j];
        }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        T12[4 * i + 3] = t[i];
        T21[4 * i + 3] = (float)(-dot3(sRinv + 3 * i, t));
        T12[12 + i] = T21[12 + i] = 0.f;
    }
    T12[15] = T21[15] = 1.f;

    float* oq = reinterpret_cast<float*>(blk + L.o_q) + it * 4;
    float* oR = reinterpret_cast<float*>(blk + L.o_R) + it * 9;
    float* o12 = reinterpret_cast<float*>(blk + L.o_T12) + it * 16;
    float* o21 = reinterpret_cast<float*>(blk + L.o_T21) + it * 16;
#pragma unroll
    for (int k = 0; k < 4; k++) oq[k] = q[k];
#pragma unroll
    for (int k = 0; k < 9; k++) oR[k] = R[k];
    reinterpret_cast<float*>(blk + L.o_s)[it] = s12;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        o12[k] = T12[k];
        o21[k] = T21[k];
    }
}

// ---------------------------------------------------------------------------
// k_sim3_check
// ---------------------------------------------------------------------------
// CheckInliers' test (:343-351) of one staged correspondence c (x3dc1 0..2,
// x3dc2 3..5, p1im1 6..7, p2im2 8..9, the limits 10..11 as floats) under the
// rows 0..2 of T12 / T21.  NaNs fail it, as in the reference.
__device__ inline bool sim3_inlier(const float* c, const float* T12, const float* T21, const float* cam1,
                                   const float* cam2, int contract)
{
    float X[3], u, v;
#pragma unroll
    for (int r = 0; r < 3; r++) X[r] = affine3(T12 + 4 * r, c + 3, T12[4 * r + 3]);
    cam_to_image(cam1, X[0], X[1], X[2], contract, u, v);   // vP2im1
    const float d1x = c[6] - u, d1y = c[7] - v;
    // dist.dot(dist) of two entries: no dot3
    const float err1 = (float)((double)d1x * (double)d1x + (double)d1y * (double)d1y);
#pragma unroll
    for (int r = 0; r < 3; r++) X[r] = affine3(T21 + 4 * r, c, T21[4 * r + 3]);
    cam_to_image(cam2, X[0], X[1], X[2], contract, u, v);   // vP1im2
    const float d2x = u - c[8], d2y = v - c[9];
    const float err2 = (float)((double)d2x * (double)d2x + (double)d2y * (double)d2y);
    return err1 < c[10] && err2 < c[11];
}

__device__ inline void sim3_stage(float* s_c, const uint8_t* blk, const Sim3Layout& L, int first, int count, int tid,
                                  int nthreads)
{
    const float* x1 = reinterpret_cast<const float*>(blk + L.o_x1);
    const float* x2 = reinterpret_cast<const float*>(blk + L.o_x2);
    const float* p1 = reinterpret_cast<const float*>(blk + L.o_p1);
    const float* p2 = reinterpret_cast<const float*>(blk + L.o_p2);
    const int32_t* l1 = reinterpret_cast<const int32_t*>(blk + L.o_l1);
    const int32_t* l2 = reinterpret_cast<const int32_t*>(blk + L.o_l2);
    for (int i = tid; i < count; i += nthreads) {
        const int g = first + i;
        float* c = s_c + i * kSim3Floats;
        c[0] = x1[3 * g];
        c[1] = x1[3 * g + 1];
        c[2] = x1[3 * g + 2];
        c[3] = x2[3 * g];
        c[4] = x2[3 * g + 1];
        c[5] = x2[3 * g + 2];
        c[6] = p1[2 * g];
        c[7] = p1[2 * g + 1];
        c[8] = p2[2 * g];
        c[9] = p2[2 * g + 1];
        c[10] = (float)l1[g];   // err < limit compares the float with the size_t as a float
        c[11] = (float)l2[g];
    }
}

__global__ __launch_bounds__(1024) void k_sim3_check(const Sim3Pair* __restrict__ descs, uint8_t* __restrict__ res,
                                                     Sim3Layout L, int contract)
{
    __shared__ float s_c[kSim3Tile * kSim3Floats];
    __shared__ int s_count[kSim3MaxIter];
    __shared__ int s_found;
    const Sim3Pair& d = descs[blockIdx.x];
    uint8_t* blk = res + (long long)blockIdx.x * L.stride;
    Sim3Hdr* hdr = reinterpret_cast<Sim3Hdr*>(blk);
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int M = min(min(d.n_iter, L.M), kSim3MaxIter);
    const int N = min(hdr->N, L.cap);
    const int n1 = max(0, min(d.n1, L.cap));
    uint8_t* inl = blk + L.o_inl;
    for (int i = tid; i < n1; i += nthreads) inl[i] = 0;
    if (!hdr->run) {   // uniform: N < min_inliers (:146-150) or a discarded candidate
        if (tid == 0) {
            hdr->iters_run = 0;
            hdr->no_more = hdr->discarded ? 0 : 1;
            hdr->found = 0;
            hdr->found_iter = -1;
            hdr->n_inliers = 0;
            hdr->best_out = d.best_in;
            hdr->best_iter = -1;
        }
        return;
    }
    const float* T12 = reinterpret_cast<const float*>(blk + L.o_T12);
    const float* T21 = reinterpret_cast<const float*>(blk + L.o_T21);
    int32_t* count = reinterpret_cast<int32_t*>(blk + L.o_cnt);
    for (int i = tid; i < M; i += nthreads) s_count[i] = 0;
    // a lane per (iteration, slice): the lanes of a wave share the
    // correspondence (LDS broadcast) and differ in the iteration
    const int S = max(1, nthreads / M);
    for (int first = 0; first < N; first += kSim3Tile) {
        const int cnt = min(kSim3Tile, N - first);
        __syncthreads();
        sim3_stage(s_c, blk, L, first, cnt, tid, nthreads);
        __syncthreads();
        for (int w = tid; w < M * S; w += nthreads) {
            const int it = w % M, slice = w / M;
            float a[12], b[12];
#pragma unroll
            for (int k = 0; k < 12; k++) {
                a[k] = T12[it * 16 + k];
                b[k] = T21[it * 16 + k];
            }
            int c = 0;
            for (int i = slice; i < cnt; i += S) c += sim3_inlier(s_c + i * kSim3Floats, a, b, d.cam1, d.cam2, contract);
            if (c) atomicAdd(&s_count[it], c);
        }
    }
    __syncthreads();
    for (int i = tid; i < M; i += nthreads) count[i] = s_count[i];
    // iterate's loop (:158-201) over the counts
    if (tid == 0) {
        const int max_its = hdr->max_its;
        const int E = max(0, min(M, max_its - d.iter_done));
        int best = d.best_in, best_iter = -1, found = -1;
        for (int it = 0; it < E; it++) {
            const int c = s_count[it];
            if (c >= best) {
                best = c;
                best_iter = it;
                if (c > d.min_inliers) {
                    found = it;
                    break;
                }
            }
        }
        const int run = found >= 0 ? found + 1 : E;
        hdr->iters_run = run;
        hdr->no_more = found < 0 && d.iter_done + run >= max_its;
        hdr->found = found >= 0;
        hdr->found_iter = found;
        hdr->n_inliers = found >= 0 ? s_count[found] : 0;
        hdr->best_out = best;
        hdr->best_iter = best_iter;
        if (best_iter >= 0) {
            const float* R = reinterpret_cast<const float*>(blk + L.o_R) + best_iter * 9;
            for (int k = 0; k < 9; k++) hdr->R12[k] = R[k];
            for (int k = 0; k < 3; k++) hdr->t12[k] = T12[best_iter * 16 + 4 * k + 3];
            hdr->s12 = reinterpret_cast<const float*>(blk + L.o_s)[best_iter];
        }
        if (found >= 0)
            for (int k = 0; k < 16; k++) hdr->T12[k] = T12[found * 16 + k];
        s_found = found;
    }
    __syncthreads();
    const int found = s_found;
    if (found < 0) return;   // uniform
    // vbInliers of the returned iteration (:195-197), recomputed
    float a[12], b[12];
#pragma unroll
    for (int k = 0; k < 12; k++) {
        a[k] = T12[found * 16 + k];
        b[k] = T21[found * 16 + k];
    }
    const int32_t* indices1 = reinterpret_cast<const int32_t*>(blk + L.o_idx);
    for (int first = 0; first < N; first += kSim3Tile) {
        const int cnt = min(kSim3Tile, N - first);
        __syncthreads();
        sim3_stage(s_c, blk, L, first, cnt, tid, nthreads);
        __syncthreads();
        for (int i = tid; i < cnt; i += nthreads)
            if (sim3_inlier(s_c + i * kSim3Floats, a, b, d.cam1, d.cam2, contract)) {
                const int i1 = indices1[first + i];
                if (i1 >= 0 && i1 < n1) inl[i1] = 1;
            }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {

int launch_sim3(orbx_ctx* ctx, int P, const Sim3Pair* descs, uint8_t* res, const Sim3Layout& L)
{
    hipStream_t st = ctx->stream;
    const int contract = ctx->fp_contract;
    timer_begin(ctx, "sim3");
    timer_begin(ctx, "sim3.prepare");
    hipLaunchKernelGGL(k_sim3_prepare, dim3(P), dim3(256), 0, st, descs, res, L, contract);
    timer_end(ctx, "sim3.prepare");
    ORBX_HIP_CHECK(hipGetLastError());
    timer_begin(ctx, "sim3.solve");
    hipLaunchKernelGGL(k_sim3_solve, dim3((L.M + 63) / 64, P), dim3(64), 0, st, descs, res, L);
    timer_end(ctx, "sim3.solve");
    ORBX_HIP_CHECK(hipGetLastError());
    timer_begin(ctx, "sim3.check");
    hipLaunchKernelGGL(k_sim3_check, dim3(P), dim3(1024), 0, st, descs, res, L, contract);
    timer_end(ctx, "sim3.check");
    timer_end(ctx, "sim3");
    ORBX_HIP_CHECK(hipGetLastError());
    return ORBX_OK;
}

// SetRansacParameters (:114-138) for N correspondences: the float epsilon,
// the double log / pow / ceil.  N < min_inliers (the reference converts a
// NaN to int) is reported as 0; a quotient past INT_MAX saturates.
int ransac_max_its(int N, int min_inliers, double probability, int max_iterations)
{
    if (N < min_inliers) return 0;
    const int nIterations = min_inliers == N ? 1 : ransac_iterations((float)min_inliers / N, probability);
    return std::max(1, std::min(nIterations, max_iterations));
}

// Stricter than orbx_pnp.hip's: the kernels convert 9.210 * sigma2 to int.
bool sigma2_ok(const float* s, int nlevels)
{
    if (!s) return false;
    for (int l = 0; l < nlevels; l++) {
        const double lim = 9.210 * (double)s[l];
        if (!(s[l] >= 0.f) || !(lim < 2147483648.0)) return false;
    }
    return true;
}

int check_params(double probability, int min_inliers, int max_iterations, int n_iter, const int32_t* draws,
                 long long n_draws, int iter_done, int best_inliers)
{
    if (n_iter < 1 || n_iter > kSim3MaxIter || !draws || min_inliers < 3 || max_iterations < 1 ||
        !(probability > 0.0 && probability < 1.0) || iter_done < 0 || best_inliers < 0)
        return ORBX_ERR_ARG;
    for (long long i = 0; i < n_draws; i++)
        if (draws[i] < 0) return ORBX_ERR_ARG;
    return ORBX_OK;
}

void rows3(const float* T, float* out) { std::memcpy(out, T, 12 * sizeof(float)); }

// One pair's result block (host copy) into the query's outputs and taps.
void scatter(const uint8_t* blk, const Sim3Layout& L, int n1, int M, orbx_sim3_query* q)
{
    const Sim3Hdr* h = reinterpret_cast<const Sim3Hdr*>(blk);
    q->N = h->N;
    q->ransac_max_its = h->max_its;
    q->iters_run = h->iters_run;
    q->no_more = h->no_more;
    q->found = h->found;
    q->found_iter = h->found_iter;
    q->n_inliers = h->n_inliers;
    q->best_inliers_out = h->best_out;
    q->best_iter = h->best_iter;
    if (h->found) std::memcpy(q->T12, h->T12, sizeof(q->T12));
    if (h->best_iter >= 0) {
        std::memcpy(q->R12, h->R12, sizeof(q->R12));
        std::memcpy(q->t12, h->t12, sizeof(q->t12));
        q->s12 = h->s12;
    }
    const int n = std::min(n1, std::min(q->cap, L.cap));
    if (q->inliers && n > 0) std::memcpy(q->inliers, blk + L.o_inl, n);
    auto tap = [&](void* dst, int off, size_t bytes) {
        if (dst && bytes) std::memcpy(dst, blk + off, bytes);
    };
    tap(q->sets, L.o_sets, (size_t)M * 12);
    tap(q->q, L.o_q, (size_t)M * 16);
    tap(q->R, L.o_R, (size_t)M * 36);
    tap(q->scale, L.o_s, (size_t)M * 4);
    tap(q->T12_all, L.o_T12, (size_t)M * 64);
    tap(q->T21_all, L.o_T21, (size_t)M * 64);
    tap(q->count, L.o_cnt, (size_t)M * 4);
    const size_t N = (size_t)std::max(0, std::min(h->N, n));
    tap(q->indices1, L.o_idx, N * 4);
    tap(q->x3dc1, L.o_x1, N * 12);
    tap(q->x3dc2, L.o_x2, N * 12);
    tap(q->p1im1, L.o_p1, N * 8);
    tap(q->p2im2, L.o_p2, N * 8);
    tap(q->max_err1, L.o_l1, N * 4);
    tap(q->max_err2, L.o_l2, N * 4);
}

}  // namespace
}  // namespace orbx

using namespace orbx;

extern "C" int orbx_sim3_ransac_batch(orbx_ctx* ctx, int B, orbx_sim3_query* qs)
{
    if (!ctx || !qs || B < 1) return ORBX_ERR_ARG;
    // argument rules, before any device work; what travels is taken as it is checked:
    // descriptors | per pair: keypoints, matches, idx1, draws, positions, sigma2, flags
    struct Staged {
        Region<orbx_keypoint> k1, k2;
        Region<int32_t> m12, idx1, draws;
        Region<float> pos1, pos2, sigma2_1, sigma2_2;
        Region<uint8_t> valid1, valid2;
    };
    int Mmax = 0, cap = 1;
    std::vector<int> Ns(B);
    std::vector<Staged> at(B);
    PackedStage st(ctx);
    const Region<Sim3Pair> descs = st.take<Sim3Pair>(B);
    for (int b = 0; b < B; b++) {
        const orbx_sim3_query& q = qs[b];
        if (q.n1 < 0 || q.n2 < 0 || (q.n1 > 0 && (!q.keys1 || !q.matches12 || !q.pos1 || !q.valid1 || !q.inliers)) ||
            (q.n2 > 0 && (!q.keys2 || !q.pos2 || !q.valid2)) || !q.T1w || !q.T2w || !q.cam1 || !q.cam2)
            return ORBX_ERR_ARG;
        int r = check_params(q.probability, q.min_inliers, q.max_iterations, q.n_iter, q.draws,
                             (long long)std::max(q.n_iter, 0) * 3, q.iter_done, q.best_inliers);
        if (r != ORBX_OK) return r;
        if (q.nlevels < 1 || q.nlevels > kMaxLevels || !sigma2_ok(q.sigma2_1, q.nlevels) || !sigma2_ok(q.sigma2_2, q.nlevels))
            return ORBX_ERR_ARG;
        if (q.n1 > kMaxFeatures || q.n2 > kMaxFeatures) return ORBX_ERR_UNSUPPORTED;
        if (!octaves_ok(q.keys1, q.n1, q.nlevels) || !octaves_ok(q.keys2, q.n2, q.nlevels)) return ORBX_ERR_ARG;
        int N = 0;
        for (int i = 0; i < q.n1; i++) {
            const int i2 = q.matches12[i];
            if (i2 >= q.n2) return ORBX_ERR_ARG;   // the reference would read past KF2's keypoints
            const int k1 = q.idx1 ? q.idx1[i] : i;
            if (q.idx1 && k1 >= q.n1) return ORBX_ERR_ARG;
            N += i2 >= 0 && k1 >= 0 && q.valid1[k1] && q.valid2[i2];
        }
        if (q.cap < q.n1) return ORBX_ERR_CAPACITY;
        Ns[b] = N;
        Mmax = std::max(Mmax, q.n_iter);
        cap = std::max(cap, q.n1);
        at[b] = {st.take(q.n1, q.keys1), st.take(q.n2, q.keys2), st.take(q.n1, q.matches12),
                 st.take(q.idx1 ? q.n1 : 0, q.idx1), st.take((size_t)q.n_iter * 3, q.draws),
                 st.take((size_t)q.n1 * 3, q.pos1), st.take((size_t)q.n2 * 3, q.pos2), st.take(q.nlevels, q.sigma2_1),
                 st.take(q.nlevels, q.sigma2_2), st.take<uint8_t>(q.n1), st.take<uint8_t>(q.n2)};
    }
    ctx_enter(ctx);
    const Sim3Layout L = sim3_layout(Mmax, cap);
    int r = st.open((size_t)B * L.stride);
    if (r != ORBX_OK) return r;
    auto flags = [&](Region<uint8_t> to, const uint8_t* src) {   // any non-zero flag is a good map point
        for (size_t i = 0; i < to.count; i++) st.host(to)[i] = src[i] ? 1 : 0;
        return st.dev(to);
    };
    for (int b = 0; b < B; b++) {
        const orbx_sim3_query& q = qs[b];
        const Staged& a = at[b];
        Sim3Pair& d = st.host(descs)[b];
        d.k1 = st.dev(a.k1);
        d.k2 = st.dev(a.k2);
        d.m12 = st.dev(a.m12);
        d.idx1 = q.idx1 ? st.dev(a.idx1) : nullptr;
        d.pos1 = st.dev(a.pos1);
        d.pos2 = st.dev(a.pos2);
        d.valid1 = flags(a.valid1, q.valid1);
        d.valid2 = flags(a.valid2, q.valid2);
        d.sigma2_1 = st.dev(a.sigma2_1);
        d.sigma2_2 = st.dev(a.sigma2_2);
        d.draws = st.dev(a.draws);
        d.its_table = nullptr;
        d.n_matches = nullptr;
        d.n1 = q.n1;
        d.n2 = q.n2;
        d.nlevels = q.nlevels;
        d.min_inliers = q.min_inliers;
        d.max_its = ransac_max_its(Ns[b], q.min_inliers, q.probability, q.max_iterations);
        d.min_matches = 0;
        d.iter_done = q.iter_done;
        d.best_in = q.best_inliers;
        d.n_iter = q.n_iter;
        rows3(q.T1w, d.T1w);
        rows3(q.T2w, d.T2w);
        std::memcpy(d.cam1, q.cam1, 16);
        std::memcpy(d.cam2, q.cam2, 16);
    }
    ResultBlocks res(ctx, st.behind(), B, L.stride);
    if ((r = st.upload()) != ORBX_OK || (r = res.zero()) != ORBX_OK) return r;
    if ((r = launch_sim3(ctx, B, st.dev(descs), res.dev, L)) != ORBX_OK) return r;
    if ((r = res.read()) != ORBX_OK) return r;
    for (int b = 0; b < B; b++) scatter(res.block(b), L, qs[b].n1, qs[b].n_iter, &qs[b]);
    return ORBX_OK;
}

extern "C" int orbx_sim3_ransac(orbx_ctx* ctx, orbx_sim3_query* q) { return orbx_sim3_ransac_batch(ctx, 1, q); }

extern "C" int orbx_dev_sim3_candidates(orbx_ctx* ctx, int slot1, const orbx_sim3_kf* kf1, int n, const int* slots2,
                                        const orbx_sim3_kf* kf2s, float nnratio, int check_ori, int min_matches,
                                        double probability, int min_inliers, int max_iterations, int n_iter,
                                        const int32_t* draws, int32_t* const* matches12, int cap, int* n_matches,
                                        int* discarded, orbx_sim3_query* out)
{
    if (!ctx || n < 0) return ORBX_ERR_ARG;
    if (n == 0) return ORBX_OK;
    auto kf_ok = [&](const orbx_sim3_kf* k) {
        return k && k->mp && k->pos && k->Tcw && k->cam && k->nlevels == ctx->geom.nlevels && k->nlevels >= 1 &&
               k->nlevels <= kMaxLevels && sigma2_ok(k->sigma2, k->nlevels);
    };
    if (!kf_ok(kf1) || !slots2 || !kf2s || !matches12 || !n_matches || !discarded || !out || min_matches < 0)
        return ORBX_ERR_ARG;
    int r = check_params(probability, min_inliers, max_iterations, n_iter, draws, (long long)std::max(n_iter, 0) * 3 * n, 0, 0);
    if (r != ORBX_OK) return r;
    for (int k = 0; k < n; k++)
        if (!kf_ok(&kf2s[k]) || !matches12[k] || !out[k].inliers || out[k].iter_done < 0 || out[k].best_inliers < 0)
            return ORBX_ERR_ARG;
    const int nf = ctx->bow_nf;
    if (nf > kMaxFeatures) return ORBX_ERR_UNSUPPORTED;
    for (int k = 0; k < n; k++)
        if (out[k].cap < nf) return ORBX_ERR_CAPACITY;
    const int nl = kf1->nlevels;
    const int len = std::max(nf, 1);
    const Sim3Layout L = sim3_layout(n_iter, len);
    // what the solver adds to the search's upload: descriptors | its table |
    // KF1: positions, sigma2 | per candidate: positions, sigma2, draws | result blocks
    struct Kf {
        Region<float> pos, sigma2;
    };
    PackedStage st(ctx);
    auto take_kf = [&](const orbx_sim3_kf& k) { return Kf{st.take<float>((size_t)len * 3), st.take(nl, k.sigma2)}; };
    const Region<Sim3Pair> descs = st.take<Sim3Pair>(n);
    const Region<int32_t> table = st.take<int32_t>(kMaxFeatures + 1);
    const Kf at1 = take_kf(*kf1);
    std::vector<Kf> at2(n);
    std::vector<Region<int32_t>> at_draws(n);
    std::vector<const uint8_t*> mp2s(n);
    for (int k = 0; k < n; k++) {
        at2[k] = take_kf(kf2s[k]);
        at_draws[k] = st.take((size_t)n_iter * 3, draws + (size_t)k * n_iter * 3);
        mp2s[k] = kf2s[k].mp;
    }
    st.align_end(256);
    BowQueued q;
    r = queue_bow_slots(ctx, 1, slot1, kf1->mp, n, slots2, mp2s.data(), nnratio, check_ori, nullptr, nullptr, 0, cap,
                        st.total + (size_t)n * L.stride, nullptr, &q);
    if (r != ORBX_OK) return r;
    // the search knows the slots' keypoint counts: that many positions of each keyframe
    st.later(at1.pos.part(0, (size_t)q.n1 * 3), kf1->pos);
    for (int k = 0; k < n; k++) st.later(at2[k].pos.part(0, (size_t)q.n2[k] * 3), kf2s[k].pos);
    st.bind(q.extra);
    for (int N = 0; N <= kMaxFeatures; N++) st.host(table)[N] = ransac_max_its(N, min_inliers, probability, max_iterations);
    for (int k = 0; k < n; k++) {
        Sim3Pair& d = st.host(descs)[k];
        d.k1 = q.k1;
        d.k2 = q.k2[k];
        d.m12 = q.out[k];
        d.idx1 = nullptr;
        d.pos1 = st.dev(at1.pos);
        d.pos2 = st.dev(at2[k].pos);
        d.valid1 = q.mp1;
        d.valid2 = q.mp2[k];
        d.sigma2_1 = st.dev(at1.sigma2);
        d.sigma2_2 = st.dev(at2[k].sigma2);
        d.draws = st.dev(at_draws[k]);
        d.its_table = st.dev(table);
        d.n_matches = q.out_n[k];
        d.n1 = q.n1;
        d.n2 = q.n2[k];
        d.nlevels = nl;
        d.min_inliers = min_inliers;
        d.max_its = -1;
        d.min_matches = min_matches;
        d.iter_done = out[k].iter_done;
        d.best_in = out[k].best_inliers;
        d.n_iter = n_iter;
        rows3(kf1->Tcw, d.T1w);
        rows3(kf2s[k].Tcw, d.T2w);
        std::memcpy(d.cam1, kf1->cam, 16);
        std::memcpy(d.cam2, kf2s[k].cam, 16);
    }
    ResultBlocks res(ctx, st.behind(), n, L.stride);
    if ((r = st.upload()) != ORBX_OK || (r = res.zero()) != ORBX_OK) return r;
    if ((r = launch_sim3(ctx, n, st.dev(descs), res.dev, L)) != ORBX_OK) return r;
    if ((r = read_bow_queued(ctx, q, q.out_len, matches12, n_matches)) != ORBX_OK) return r;
    if ((r = res.read()) != ORBX_OK) return r;
    for (int k = 0; k < n; k++) {
        if (n_matches[k] < 0) return ORBX_ERR_UNSUPPORTED;
        const uint8_t* blk = res.block(k);
        discarded[k] = reinterpret_cast<const Sim3Hdr*>(blk)->discarded;
        scatter(blk, L, q.n1, n_iter, &out[k]);
    }
    return ORBX_OK;
}
