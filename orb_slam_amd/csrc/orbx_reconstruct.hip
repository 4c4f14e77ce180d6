// The end of map initialisation on the device: Initializer::Initialize after
// the score ratio (src/Initializer.cc:113-119) -- ReconstructH (:570-730) or
// ReconstructF (:468-568) with CheckRT (:796-905), Triangulate (:732-745) and
// DecomposeE (:907-927).
//
// Three kernels per call, each over all pairs of the call:
//   k_rec_hyp     a lane per pair: E21 = Kt F21 K or A = invK H21 K, the FP64
//                 3x3 SVD (one-sided Jacobi, orbx_jacobi.h) rounded once, and
//                 the 4 (DecomposeE) or 8 (Faugeras) motion hypotheses with
//                 P2 = K [R|t] and O2 = -Rt t of each.
//   k_rec_check   a lane per (pair, hypothesis, match index): Triangulate and
//                 CheckRT's gates in the reference's order; A and V of the 4x4
//                 null vector in the lane's registers (32 doubles), as in
//                 k_triangulate.  The cosine, the candidate point and its
//                 flag are stored by match index.
//   k_rec_select  a workgroup per pair: per hypothesis nGood (an integer
//                 atomic in LDS over the stored cosines), the cosine at
//                 sorted position min(50, nGood - 1) by rank count in LDS,
//                 the parallax, the reference's decision, and the winner's
//                 points and flags scattered to their keypoints.
//
// Everything but what goes through OpenCV in the reference is its float
// arithmetic operation by operation; DESIGN.md section 4 lists the defined
// parts (the two decompositions, FP64 products / norm / dot / determinant
// rounded once).  tests/reconstruct_numpy.py restates all of it.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "orbx_device.h"
#include "orbx_init_layout.h"
#include "orbx_internal.h"
#include "orbx_jacobi.h"
#include "orbx_linalg.h"
#include "orbx_stage.h"

namespace orbx {

constexpr int kRecMaxHyp = 8;
constexpr double kRecRankCut = 1e-6;   // sigma3 <= cut * sigma1: U's third column is u1 x u2

struct RecHdr {
    int32_t ok, n_inl, n_hyp, best, model, N, n1, pad0;
    float R21[9], t21[3];
    int32_t n_good[kRecMaxHyp];
    float parallax[kRecMaxHyp];
    float svd[21], th2, pad1[2];
    float R_all[kRecMaxHyp * 9], t_all[kRecMaxHyp * 3];
    float P2[kRecMaxHyp * 12], O2[kRecMaxHyp * 3];
};
static_assert(sizeof(RecHdr) % 16 == 0, "result arrays are 16-byte aligned");

// One pair's inputs.  Host forms: compacted on the host, N / model / M21
// here.  Device-resident form: `init` is the pair's block of the models run,
// which holds N, RH and the models; n1_ptr the reference frame's count.
struct RecPair {
    const float4* xy;         // [N] (u1, v1, u2, v2) by match index
    const int2* pairs;        // [N] (i1, i2)
    const uint8_t* inl_h;     // [N] vbMatchesInliers of either model
    const uint8_t* inl_f;
    const InitHdr* init;
    const int32_t* n1_ptr;
    int32_t N, n1, model, min_tri;
    float M21[9], cam[4], sigma, min_parallax;
};

struct RecLayout {
    long long stride, o_v4, o_cos, o_pts, o_flag, o_p3d, o_tri;
    int cap;   // keypoints (and so matches) a block is sized for
};

static RecLayout rec_layout(int cap)
{
    RecLayout L;
    BlockOffsets o;
    o.take(sizeof(RecHdr));
    L.o_v4 = o.take((long long)kRecMaxHyp * cap * 16);
    L.o_cos = o.take((long long)kRecMaxHyp * cap * 4);
    L.o_pts = o.take((long long)kRecMaxHyp * cap * 12);
    L.o_flag = o.take((long long)kRecMaxHyp * cap);
    L.o_p3d = o.take((long long)cap * 12);
    L.o_tri = o.take(cap);
    L.stride = o.end;
    L.cap = cap;
    return L;
}

// ---------------------------------------------------------------------------
// defined arithmetic of the hypotheses
// ---------------------------------------------------------------------------
__device__ __forceinline__ void rec_swap_cols(JacobiCols<3>& m, double (&n)[3], int p, int q)
{
    if (n[q] > n[p]) {
        const double t = n[p];
        n[p] = n[q];
        n[q] = t;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double tb = m.a[p][i], tv = m.v[p][i];
            m.a[p][i] = m.a[q][i];
            m.a[q][i] = tb;
            m.v[p][i] = m.v[q][i];
            m.v[q][i] = tv;
        }
    }
}

// U (9), w (3), Vt (9) of a row-major float 3x3: one-sided Jacobi on its
// columns in FP64 (M V = U S, orbx_jacobi.h), singular values descending
// (equal ones in column order), rounded once.  Where sigma3 <= kRecRankCut
// sigma1 -- always, for an essential matrix formed in float -- the third
// column of U is the cross product of the first two instead of a column of
// round-off divided by its norm.
__device__ inline void svd3(const float* mf, float* out)
{
    JacobiCols<3> m = hestenes(load_cols<3>(mf));
    double nrm[3];
#pragma unroll
    for (int j = 0; j < 3; j++) nrm[j] = col_dot(m.a[j], m.a[j]);
    rec_swap_cols(m, nrm, 0, 1);
    rec_swap_cols(m, nrm, 1, 2);
    rec_swap_cols(m, nrm, 0, 1);
    double s[3], u[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        s[j] = sqrt(nrm[j]);
#pragma unroll
        for (int i = 0; i < 3; i++) u[j][i] = m.a[j][i] / s[j];
    }
    if (s[2] <= kRecRankCut * s[0]) {
        u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
        u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
        u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        out[9 + j] = (float)s[j];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            out[3 * i + j] = (float)u[j][i];          // U's column j
            out[12 + 3 * j + i] = (float)m.v[j][i];   // Vt's row j
        }
    }
}

// t / cv::norm(t): a scaled convert with the float scale 1 / norm
__device__ inline void unit3(float* t)
{
    const float sc = (float)(1.0 / norm3(t));
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = t[i] * sc;
}

// R, t of one hypothesis with P2 = K*[R|t] (:819-822) and O2 = -R.t()*t (:824)
__device__ inline void store_hyp(RecHdr* h, int k, const float* cam, const float* R, const float* t)
{
    const float K[9] = {cam[0], 0.f, cam[2], 0.f, cam[1], cam[3], 0.f, 0.f, 1.f};
#pragma unroll
    for (int i = 0; i < 9; i++) h->R_all[9 * k + i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) h->t_all[3 * k + i] = t[i];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float r0 = j < 3 ? R[j] : t[0], r1 = j < 3 ? R[3 + j] : t[1], r2 = j < 3 ? R[6 + j] : t[2];
            h->P2[12 * k + 4 * i + j] = (float)dot3(K + 3 * i, r0, r1, r2);
        }
#pragma unroll
    for (int i = 0; i < 3; i++) h->O2[3 * k + i] = (float)(-dot3(t, R[i], R[3 + i], R[6 + i]));
}

// ---------------------------------------------------------------------------
// k_rec_hyp
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_rec_hyp(const RecPair* __restrict__ descs, uint8_t* __restrict__ res,
                                                RecLayout L, int P, float rh_threshold, int contract)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const RecPair& d = descs[p];
    RecHdr* h = reinterpret_cast<RecHdr*>(res + (long long)p * L.stride);
    int N = d.N, model = d.model;
    bool valid = true;
    float M[9];
    if (d.init) {
        N = d.init->n;
        valid = N >= 8 && d.init->best_h >= 0 && d.init->best_f >= 0;
        model = d.init->RH > rh_threshold ? 0 : 1;   // :113
#pragma unroll
        for (int i = 0; i < 9; i++) M[i] = model ? d.init->F21[i] : d.init->H21[i];
    } else {
#pragma unroll
        for (int i = 0; i < 9; i++) M[i] = d.M21[i];
    }
    const int n1 = max(0, min(d.n1_ptr ? *d.n1_ptr : d.n1, L.cap));
    N = max(0, min(N, n1));
    valid = valid && N > 0;
    h->ok = 0;
    h->n_inl = 0;
    h->n_hyp = 0;
    h->best = -1;
    h->model = model;
    h->N = N;
    h->n1 = n1;
    h->pad0 = 0;
    const float sigma2 = d.sigma * d.sigma;            // mSigma2 (:40)
    h->th2 = (float)(4.0 * (double)sigma2);            // 4.0*mSigma2 into CheckRT's float th2
    h->pad1[0] = h->pad1[1] = 0.f;
    for (int i = 0; i < 9; i++) h->R21[i] = 0.f;
    for (int i = 0; i < 3; i++) h->t21[i] = 0.f;
    for (int i = 0; i < kRecMaxHyp; i++) {
        h->n_good[i] = 0;
        h->parallax[i] = 0.f;
    }
    for (int i = 0; i < 21; i++) h->svd[i] = 0.f;
    for (int i = 0; i < kRecMaxHyp * 9; i++) h->R_all[i] = 0.f;
    for (int i = 0; i < kRecMaxHyp * 3; i++) h->t_all[i] = 0.f;
    for (int i = 0; i < kRecMaxHyp * 12; i++) h->P2[i] = 0.f;
    for (int i = 0; i < kRecMaxHyp * 3; i++) h->O2[i] = 0.f;
    if (!valid) return;

    const float K[9] = {d.cam[0], 0.f, d.cam[2], 0.f, d.cam[1], d.cam[3], 0.f, 0.f, 1.f};
    float S[21], tmp[9], X[9];
    if (model) {   // E21 = K.t()*F21*K (:477)
        const float Kt[9] = {d.cam[0], 0.f, 0.f, 0.f, d.cam[1], 0.f, d.cam[2], d.cam[3], 1.f};
        mul3(Kt, M, tmp);
        mul3(tmp, K, X);
    } else {       // A = invK*H21*K (:582-583)
        float invK[9];
        inv3(K, invK);
        mul3(invK, M, tmp);
        mul3(tmp, K, X);
    }
    svd3(X, S);
    for (int i = 0; i < 21; i++) h->svd[i] = S[i];
    const float* U = S;
    const float* w = S + 9;
    const float* Vt = S + 12;

    if (model) {
        // DecomposeE (:907-927); hypotheses (R1,t), (R2,t), (R1,-t), (R2,-t) (:492-495)
        float t[3] = {U[2], U[5], U[8]};
        unit3(t);
        const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
        const float Wt[9] = {0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
        float R1[9], R2[9];
        mul3(U, W, tmp);
        mul3(tmp, Vt, R1);
        if (det3(R1) < 0.0)
            for (int i = 0; i < 9; i++) R1[i] = -R1[i];
        mul3(U, Wt, tmp);
        mul3(tmp, Vt, R2);
        if (det3(R2) < 0.0)
            for (int i = 0; i < 9; i++) R2[i] = -R2[i];
        const float tn[3] = {-t[0], -t[1], -t[2]};
        store_hyp(h, 0, d.cam, R1, t);
        store_hyp(h, 1, d.cam, R2, t);
        store_hyp(h, 2, d.cam, R1, tn);
        store_hyp(h, 3, d.cam, R2, tn);
        h->n_hyp = 4;
        return;
    }

    // ReconstructH (:589-684)
    const float s = (float)(det3(U) * det3(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return;   // :595-598
    float d12, d23, d13, c_num, p_num;
    if (contract) {
        d12 = fmaf(d1, d1, -(d2 * d2));
        d23 = fmaf(d2, d2, -(d3 * d3));
        d13 = fmaf(d1, d1, -(d3 * d3));
        c_num = fmaf(d2, d2, d1 * d3);
        p_num = fmaf(d1, d3, -(d2 * d2));
    } else {
        d12 = d1 * d1 - d2 * d2;
        d23 = d2 * d2 - d3 * d3;
        d13 = d1 * d1 - d3 * d3;
        c_num = d2 * d2 + d1 * d3;
        p_num = d1 * d3 - d2 * d2;
    }
    const float aux1 = sqrtf(d12 / d13);
    const float aux3 = sqrtf(d23 / d13);
    const float root = sqrtf(d12 * d23);
    const float aux_stheta = root / ((d1 + d3) * d2);
    const float ctheta = c_num / ((d1 + d3) * d2);
    const float aux_sphi = root / ((d1 - d3) * d2);
    const float cphi = p_num / ((d1 - d3) * d2);
    for (int i = 0; i < 4; i++) {
        const float x1 = i < 2 ? aux1 : -aux1;
        const float x3 = (i & 1) ? -aux3 : aux3;
        const float st = (i == 0 || i == 3) ? aux_stheta : -aux_stheta;
        const float sp = (i == 0 || i == 3) ? aux_sphi : -aux_sphi;
        float R[9], t[3];
        {   // case d' = d2 (:617-646)
            const float Rp[9] = {ctheta, 0.f, -st, 0.f, 1.f, 0.f, st, 0.f, ctheta};
            scaled_mul3(s, U, Rp, tmp);
            mul3(tmp, Vt, R);
            const float sc = d1 - d3;
            const float tp[3] = {x1 * sc, 0.f, -x3 * sc};
            matvec3(U, tp, t);
            unit3(t);
            store_hyp(h, i, d.cam, R, t);
        }
        {   // case d' = -d2 (:654-684)
            const float Rp[9] = {cphi, 0.f, sp, 0.f, -1.f, 0.f, sp, 0.f, -cphi};
            scaled_mul3(s, U, Rp, tmp);
            mul3(tmp, Vt, R);
            const float sc = d1 + d3;
            const float tp[3] = {x1 * sc, 0.f, x3 * sc};
            matvec3(U, tp, t);
            unit3(t);
            store_hyp(h, 4 + i, d.cam, R, t);
        }
    }
    h->n_hyp = 8;
}

// ---------------------------------------------------------------------------
// k_rec_check
// ---------------------------------------------------------------------------
// The reprojection gate of one image (:865-884): true = rejected.
__device__ inline bool rec_reproj_rejects(const float* cam, const float* pt, float u, float v, float th2, int contract)
{
    return reproj_e2(cam, pt[0], pt[1], pt[2], u, v, contract) > th2;
}

__global__ __launch_bounds__(256) void k_rec_check(const RecPair* __restrict__ descs, uint8_t* __restrict__ res,
                                                   RecLayout L, int contract)
{
    // pairs along x: consecutive workgroups go to different XCDs, and the
    // chunks of match indices past a pair's N (most of them) are empty
    const int p = blockIdx.x, hyp = blockIdx.y;
    const int i = blockIdx.z * blockDim.x + threadIdx.x;
    uint8_t* blk = res + (long long)p * L.stride;
    RecHdr* h = reinterpret_cast<RecHdr*>(blk);
    if (hyp >= h->n_hyp || i >= h->N) return;   // N <= n1 <= L.cap (k_rec_hyp)
    const RecPair& d = descs[p];
    const long long at = (long long)hyp * L.cap + i;
    float* o_v4 = reinterpret_cast<float*>(blk + L.o_v4) + 4 * at;
    float* o_cos = reinterpret_cast<float*>(blk + L.o_cos) + at;
    float* o_pt = reinterpret_cast<float*>(blk + L.o_pts) + 3 * at;
    uint8_t* o_flag = blk + L.o_flag + at;
    const uint8_t inl = (h->model ? d.inl_f : d.inl_h)[i];
    float v4[4] = {0.f, 0.f, 0.f, 0.f}, x[3] = {0.f, 0.f, 0.f};
    float cosv = __builtin_nanf("");
    int flag = 0;   // 1: counted (:886-888), 2: counted and triangulated (:890-891)
    if (inl) {
        const float4 m = d.xy[i];
        const float* cam = d.cam;
        const float* P2 = h->P2 + 12 * hyp;
        const float* O2 = h->O2 + 3 * hyp;
        const float* R = h->R_all + 9 * hyp;
        const float* t = h->t_all + 3 * hyp;
        // Triangulate (:732-745): P1 = K[I|0]
        float A[16];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float p10 = j == 0 ? cam[0] : (j == 2 ? cam[2] : 0.f);
            const float p11 = j == 1 ? cam[1] : (j == 2 ? cam[3] : 0.f);
            const float p12 = j == 2 ? 1.f : 0.f;
            A[j] = m.x * p12 - p10;
            A[4 + j] = m.y * p12 - p11;
            A[8 + j] = m.z * P2[8 + j] - P2[j];
            A[12 + j] = m.w * P2[8 + j] - P2[4 + j];
        }
        null_vector4(A, v4);
        const float inv = (float)(1.0 / (double)v4[3]);
        x[0] = v4[0] * inv;
        x[1] = v4[1] * inv;
        x[2] = v4[2] * inv;
        bool alive = isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);   // :839
        // parallax (:846-852); O1 = 0
        const float dist1 = (float)norm3(x);
        const float n2[3] = {x[0] - O2[0], x[1] - O2[1], x[2] - O2[2]};
        const float dist2 = (float)norm3(n2);
        // the quotient by the float product of the rounded norms (new points divide by the double product)
        const float c = (float)(dot3(x, n2) / (double)(dist1 * dist2));
        const bool low = (double)c < 0.99998;
        if (x[2] <= 0.f && low) alive = false;                              // :855
        // p3dC2 = R*p3dC1+t (:859)
        float x2[3];
#pragma unroll
        for (int r = 0; r < 3; r++) x2[r] = affine3(R + 3 * r, x, t[r]);
        if (x2[2] <= 0.f && low) alive = false;                             // :861
        if (rec_reproj_rejects(cam, x, m.x, m.y, h->th2, contract)) alive = false;    // :872
        if (rec_reproj_rejects(cam, x2, m.z, m.w, h->th2, contract)) alive = false;   // :883
        if (alive) {
            cosv = c;
            flag = low ? 2 : 1;
        } else {
            x[0] = x[1] = x[2] = 0.f;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) o_v4[k] = v4[k];
    *o_cos = cosv;
#pragma unroll
    for (int k = 0; k < 3; k++) o_pt[k] = x[k];
    *o_flag = (uint8_t)flag;
}

// ---------------------------------------------------------------------------
// k_rec_select
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rec_select(const RecPair* __restrict__ descs, uint8_t* __restrict__ res,
                                                    RecLayout L)
{
    extern __shared__ float s_c[];   // [cap] cosines of one hypothesis
    __shared__ float s_val;
    __shared__ int s_inl, s_cnt, s_ok, s_best;
    const int p = blockIdx.x, tid = threadIdx.x;
    const RecPair& d = descs[p];
    uint8_t* blk = res + (long long)p * L.stride;
    RecHdr* h = reinterpret_cast<RecHdr*>(blk);
    const int N = h->N, n1 = h->n1, nh = h->n_hyp, model = h->model;
    const float* cosv = reinterpret_cast<const float*>(blk + L.o_cos);
    if (tid == 0) s_inl = 0;
    __syncthreads();
    {
        const uint8_t* inl = model ? d.inl_f : d.inl_h;
        int cnt = 0;
        for (int i = tid; i < N; i += blockDim.x) cnt += inl[i] != 0;
        if (cnt) atomicAdd(&s_inl, cnt);
    }
    // nGood and the parallax of every hypothesis (:886-902): the cosines that
    // reached :886 are counted (an integer atomic in LDS: exact in any order),
    // and the one at sorted position min(50, nGood - 1) is found by a rank
    // count, since only its value matters
    for (int k = 0; k < nh; k++) {
        __syncthreads();
        if (tid == 0) {
            s_val = 0.f;
            s_cnt = 0;
        }
        __syncthreads();
        int cnt = 0;
        for (int i = tid; i < N; i += blockDim.x) {
            const float c = cosv[(long long)k * L.cap + i];
            s_c[i] = c;
            cnt += c == c;
        }
        if (cnt) atomicAdd(&s_cnt, cnt);
        __syncthreads();
        const int nGood = s_cnt;
        if (nGood > 0) {
            const int idx = min(50, nGood - 1);
            for (int i = tid; i < N; i += blockDim.x) {
                const float c = s_c[i];
                if (c != c) continue;
                int rank = 0;
                for (int j = 0; j < N; j++) {
                    const float o = s_c[j];
                    rank += (o < c) || (o == c && j < i);
                }
                if (rank == idx) s_val = c;
            }
        }
        __syncthreads();
        if (tid == 0) {
            float par = 0.f;
            if (nGood > 0) {
                // acos(float) is std::acos(float) in the reference (section 4): the correctly rounded float
                const float a = (float)acos((double)s_val);
                par = (float)((double)(a * 180.f) / 3.1415926535897932384626433832795);
            }
            h->n_good[k] = nGood;
            h->parallax[k] = par;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int Ninl = s_inl;
        int ok = 0, best = -1;
        if (nh > 0 && model) {
            // ReconstructF (:497-567)
            int g[4], maxGood = 0;
            for (int k = 0; k < 4; k++) {
                g[k] = h->n_good[k];
                maxGood = max(maxGood, g[k]);
            }
            const int nMinGood = max((int)(0.9 * (double)Ninl), d.min_tri);
            int nsimilar = 0;
            for (int k = 0; k < 4; k++) nsimilar += (double)g[k] > 0.7 * (double)maxGood;
            if (!(maxGood < nMinGood || nsimilar > 1)) {
                int k = 0;
                while (g[k] != maxGood) k++;
                if (h->parallax[k] > d.min_parallax) {
                    ok = 1;
                    best = k;
                }
            }
        } else if (nh > 0) {
            // ReconstructH (:687-729)
            int bestGood = 0, secondBestGood = 0, bestIdx = -1;
            float bestParallax = -1.f;
            for (int k = 0; k < 8; k++) {
                const int nGood = h->n_good[k];
                if (nGood > bestGood) {
                    secondBestGood = bestGood;
                    bestGood = nGood;
                    bestIdx = k;
                    bestParallax = h->parallax[k];
                } else if (nGood > secondBestGood) {
                    secondBestGood = nGood;
                }
            }
            if ((double)secondBestGood < 0.75 * (double)bestGood && bestParallax >= d.min_parallax &&
                bestGood > d.min_tri && (double)bestGood > 0.9 * (double)Ninl) {
                ok = 1;
                best = bestIdx;
            }
        }
        h->ok = ok;
        h->best = best;
        h->n_inl = Ninl;
        if (ok) {
            for (int i = 0; i < 9; i++) h->R21[i] = h->R_all[9 * best + i];
            for (int i = 0; i < 3; i++) h->t21[i] = h->t_all[3 * best + i];
        }
        s_ok = ok;
        s_best = best;
    }
    __syncthreads();
    // vP3D / vbTriangulated of the winner, by keypoint of frame 1
    float* p3d = reinterpret_cast<float*>(blk + L.o_p3d);
    uint8_t* tri = blk + L.o_tri;
    for (int i = tid; i < 3 * n1; i += blockDim.x) p3d[i] = 0.f;
    for (int i = tid; i < n1; i += blockDim.x) tri[i] = 0;
    __syncthreads();
    if (!s_ok) return;
    const long long base = (long long)s_best * L.cap;
    const float* pts = reinterpret_cast<const float*>(blk + L.o_pts) + 3 * base;
    const uint8_t* flag = blk + L.o_flag + base;
    for (int i = tid; i < N; i += blockDim.x) {
        const int f = flag[i];
        const int i1 = d.pairs[i].x;
        if (f && i1 >= 0 && i1 < n1) {
            p3d[3 * i1] = pts[3 * i];
            p3d[3 * i1 + 1] = pts[3 * i + 1];
            p3d[3 * i1 + 2] = pts[3 * i + 2];
            tri[i1] = f == 2;
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {

int launch_reconstruct(orbx_ctx* ctx, int P, const RecPair* descs, uint8_t* res, const RecLayout& L, float rh_threshold)
{
    if (P <= 0) return ORBX_OK;
    hipStream_t st = ctx->stream;
    const int contract = ctx->fp_contract;
    timer_begin(ctx, "reconstruct");
    hipLaunchKernelGGL(k_rec_hyp, dim3((P + 63) / 64), dim3(64), 0, st, descs, res, L, P, rh_threshold, contract);
    hipLaunchKernelGGL(k_rec_check, dim3(P, kRecMaxHyp, (L.cap + 255) / 256), dim3(256), 0, st, descs, res, L, contract);
    hipLaunchKernelGGL(k_rec_select, dim3(P), dim3(256), (size_t)L.cap * sizeof(float), st, descs, res, L);
    timer_end(ctx, "reconstruct");
    ORBX_HIP_CHECK(hipGetLastError());
    return ORBX_OK;
}

// One pair's result block (host copy) into the query's outputs and taps.
void scatter(const uint8_t* blk, const RecLayout& L, orbx_reconstruct_query* q)
{
    const RecHdr* h = reinterpret_cast<const RecHdr*>(blk);
    q->ok = h->ok;
    q->n_inliers = h->n_inl;
    q->n_hyp = h->n_hyp;
    q->best = h->best;
    if (h->ok) {
        std::memcpy(q->R21, h->R21, sizeof(q->R21));
        std::memcpy(q->t21, h->t21, sizeof(q->t21));
    }
    std::memcpy(q->n_good, h->n_good, sizeof(q->n_good));
    std::memcpy(q->parallax, h->parallax, sizeof(q->parallax));
    const int n1 = h->n1, N = h->N;
    if (n1 > 0) {
        std::memcpy(q->p3d, blk + L.o_p3d, (size_t)n1 * 12);
        std::memcpy(q->triangulated, blk + L.o_tri, (size_t)n1);
    }
    if (q->svd) std::memcpy(q->svd, h->svd, sizeof(h->svd));
    if (q->R_all) std::memcpy(q->R_all, h->R_all, sizeof(h->R_all));
    if (q->t_all) std::memcpy(q->t_all, h->t_all, sizeof(h->t_all));
    for (int k = 0; k < h->n_hyp; k++) {
        const size_t at = (size_t)k * L.cap;
        if (q->v4) std::memcpy(q->v4 + (size_t)k * N * 4, blk + L.o_v4 + at * 16, (size_t)N * 16);
        if (q->cos_parallax) std::memcpy(q->cos_parallax + (size_t)k * N, blk + L.o_cos + at * 4, (size_t)N * 4);
    }
}

}  // namespace
}  // namespace orbx

using namespace orbx;

extern "C" int orbx_init_reconstruct_batch(orbx_ctx* ctx, int B, orbx_reconstruct_query* qs)
{
    if (!ctx || !qs || B < 1) return ORBX_ERR_ARG;
    // argument rules, before any device work
    int cap = 1;
    size_t n_m = 0;
    std::vector<int> Ns(B);
    for (int b = 0; b < B; b++) {
        const orbx_reconstruct_query& q = qs[b];
        if (q.n1 < 0 || q.n2 < 0 || (q.n1 > 0 && (!q.keys1 || !q.matches12 || !q.p3d || !q.triangulated)) ||
            (q.n2 > 0 && !q.keys2) || !q.M21 || !q.cam)
            return ORBX_ERR_ARG;
        if (q.model < 0 || q.model > 1 || !(q.sigma > 0.f)) return ORBX_ERR_ARG;
        if (q.n1 > kMaxFeatures || q.n2 > kMaxFeatures) return ORBX_ERR_UNSUPPORTED;
        int N = 0;
        for (int i = 0; i < q.n1; i++) {
            if (q.matches12[i] >= q.n2) return ORBX_ERR_ARG;   // the reference would index past mvKeys2
            N += q.matches12[i] >= 0;
        }
        if (N > 0 && !q.inliers) return ORBX_ERR_ARG;
        if (q.cap < q.n1) return ORBX_ERR_CAPACITY;
        Ns[b] = N;
        n_m += (size_t)N;
        cap = std::max(cap, q.n1);
    }
    ctx_enter(ctx);
    const RecLayout L = rec_layout(cap);
    // one upload: descriptors | (u1, v1, u2, v2) | (i1, i2) | inliers (each array the queries' end to end)
    PackedStage st(ctx);
    const Region<RecPair> descs = st.take<RecPair>(B);
    const Region<float4> xys = st.take<float4>(n_m);
    const Region<int2> prs = st.take<int2>(n_m);
    const Region<uint8_t> inl = st.take<uint8_t>(n_m);
    int r = st.open((size_t)B * L.stride);
    if (r != ORBX_OK) return r;
    size_t mm = 0;
    for (int b = 0; b < B; b++) {
        const orbx_reconstruct_query& q = qs[b];
        RecPair& d = st.host(descs)[b];
        d.xy = st.dev(xys) + mm;
        d.pairs = st.dev(prs) + mm;
        d.inl_h = d.inl_f = st.dev(inl) + mm;
        d.init = nullptr;
        d.n1_ptr = nullptr;
        d.N = Ns[b];
        d.n1 = q.n1;
        d.model = q.model;
        d.min_tri = q.min_triangulated;
        std::memcpy(d.M21, q.M21, sizeof(d.M21));
        std::memcpy(d.cam, q.cam, sizeof(d.cam));
        d.sigma = q.sigma;
        d.min_parallax = q.min_parallax;
        // mvMatches12 in i1 order (:54-63)
        float* xy = reinterpret_cast<float*>(st.host(xys) + mm);
        int32_t* pr = reinterpret_cast<int32_t*>(st.host(prs) + mm);
        int k = 0;
        for (int i = 0; i < q.n1; i++) {
            const int j = q.matches12[i];
            if (j < 0) continue;
            xy[4 * k] = q.keys1[i].x;
            xy[4 * k + 1] = q.keys1[i].y;
            xy[4 * k + 2] = q.keys2[j].x;
            xy[4 * k + 3] = q.keys2[j].y;
            pr[2 * k] = i;
            pr[2 * k + 1] = j;
            k++;
        }
        if (Ns[b]) std::memcpy(st.host(inl) + mm, q.inliers, (size_t)Ns[b]);
        mm += (size_t)Ns[b];
    }
    ResultBlocks res(ctx, st.behind(), B, L.stride);
    if ((r = st.upload()) != ORBX_OK) return r;
    if ((r = launch_reconstruct(ctx, B, st.dev(descs), res.dev, L, 0.f)) != ORBX_OK) return r;
    if ((r = res.read()) != ORBX_OK) return r;
    for (int b = 0; b < B; b++) scatter(res.block(b), L, &qs[b]);
    return ORBX_OK;
}

extern "C" int orbx_init_reconstruct(orbx_ctx* ctx, orbx_reconstruct_query* q)
{
    return orbx_init_reconstruct_batch(ctx, 1, q);
}

extern "C" int orbx_dev_init_reconstruct(orbx_ctx* ctx, int first, int count, int seq_len, const float* cam,
                                         float rh_threshold, float min_parallax, int min_triangulated)
{
    if (!ctx || !cam || seq_len < 1) return ORBX_ERR_ARG;
    // the pairs of the models run on the same slot range
    if (ctx->init_count == 0 || first != ctx->init_first || count != ctx->init_count) return ORBX_ERR_ARG;
    for (int k = 0; k < count; k++)
        if (((first + k) % seq_len == 0) != (ctx->init_pair[k] < 0)) return ORBX_ERR_ARG;
    ctx_enter(ctx);
    const int nf = std::max(ctx->geom.nfeatures, 1);
    const InitLayout IL = make_layout(ctx->init_iter, nf);
    const RecLayout L = rec_layout(nf);
    std::vector<RecPair> descs;
    for (int k = 0; k < count; k++) {
        if (ctx->init_pair[k] < 0) continue;
        const int s = first + k;
        uint8_t* blk = static_cast<uint8_t*>(ctx->init_res) + (size_t)ctx->init_pair[k] * IL.stride;
        RecPair d{};
        d.xy = reinterpret_cast<const float4*>(blk + IL.o_xy);
        d.pairs = reinterpret_cast<const int2*>(blk + IL.o_pairs);
        d.inl_h = blk + IL.o_inh;
        d.inl_f = blk + IL.o_inf;
        d.init = reinterpret_cast<const InitHdr*>(blk);
        d.n1_ptr = ctx->out_n + (s - 1);
        d.min_tri = min_triangulated;
        std::memcpy(d.cam, cam, sizeof(d.cam));
        d.sigma = ctx->init_sigma;
        d.min_parallax = min_parallax;
        descs.push_back(d);   // block init_pair[k] of the run: the same order
    }
    const int P = (int)descs.size();
    ctx->rec_count = 0;
    if ((size_t)P * L.stride > ctx->rec_res_bytes) {
        if (ctx->rec_res) (void)hipFree(ctx->rec_res);
        ctx->rec_res = nullptr;
        ctx->rec_res_bytes = 0;
        if (hipMalloc(&ctx->rec_res, (size_t)P * L.stride) != hipSuccess) return ORBX_ERR_NOMEM;
        ctx->rec_res_bytes = (size_t)P * L.stride;
    }
    if (P > 0) {
        PackedStage st(ctx);
        const Region<RecPair> pairs = st.take(P, descs.data());
        int r;
        if ((r = st.open(0)) != ORBX_OK || (r = st.upload()) != ORBX_OK) return r;
        // the blob is freed on return: the copy is waited for, the kernels are not
        ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        r = launch_reconstruct(ctx, P, st.dev(pairs), static_cast<uint8_t*>(ctx->rec_res), L, rh_threshold);
        if (r != ORBX_OK) return r;
    }
    ctx->rec_first = first;
    ctx->rec_count = count;
    ctx->rec_cap = nf;
    return ORBX_OK;
}

extern "C" int orbx_dev_read_init_reconstruct(orbx_ctx* ctx, int slot, orbx_reconstruct_query* out, int* model)
{
    if (!ctx || !out || ctx->rec_count == 0 || slot < ctx->rec_first || slot >= ctx->rec_first + ctx->rec_count)
        return ORBX_ERR_ARG;
    const int p = ctx->init_pair[slot - ctx->rec_first];
    if (p < 0) return ORBX_ERR_ARG;   // a sequence start has no pair
    ctx_enter(ctx);
    const RecLayout L = rec_layout(ctx->rec_cap);
    ResultBlocks blk(ctx, static_cast<uint8_t*>(ctx->rec_res) + (size_t)p * L.stride, 1, L.stride);
    const int r = blk.read();
    if (r != ORBX_OK) return r;
    const RecHdr* h = reinterpret_cast<const RecHdr*>(blk.block(0));
    if (model) *model = h->model;
    if (h->n1 > 0 && (!out->p3d || !out->triangulated)) return ORBX_ERR_ARG;
    if (out->cap < h->n1) return ORBX_ERR_CAPACITY;
    scatter(blk.block(0), L, out);
    return ORBX_OK;
}
