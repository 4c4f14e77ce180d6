// Map initialisation models on the device: Initializer::Initialize up to the
// score ratio (src/Initializer.cc:44-113) -- match compaction, the RANSAC
// sets from the caller's rand() draws, Normalize, and for every iteration
// ComputeH21 / ComputeF21, the denormalising products, CheckHomography /
// CheckFundamental and the selection of the best model of each kind.
//
// Three kernels per call, each over all pairs of the call:
//   k_init_prepare  a workgroup per pair: keypoint coordinates staged in LDS,
//                   then wave 0 runs Normalize's sequential float sums (a lane
//                   per frame axis) while wave 1 compacts the matches (ballot
//                   prefix), then a thread per iteration draws its set.
//   k_init_solve    a 16-lane row per hypothesis (H and F alike): lane r holds
//                   row r of A and row r of V in FP64 registers, one-sided
//                   Jacobi on A's columns with the column dot products reduced
//                   across the row; V's column of the smallest column norm is
//                   the null vector.  Then Fpre's 3x3 SVD (Jacobi again), the
//                   denormalising products and H21's inverse.
//   k_init_score    a workgroup per pair: the compacted (u1, v1, u2, v2) in
//                   LDS, a lane per (model, iteration) walking the matches in
//                   order (LDS broadcast reads), the first-strict-maximum
//                   selection, and the inlier bytes of the two winners.
//
// Everything but the two null-vector solves is float arithmetic operation by
// operation as the reference writes it (DESIGN.md section 4 lists the defined
// parts: the FP64 solves, inverses by adjugate and products rounded once).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "orbx_device.h"
#include "orbx_internal.h"
#include "orbx_init_layout.h"
#include "orbx_jacobi.h"
#include "orbx_linalg.h"
#include "orbx_stage.h"

namespace orbx {

// ---------------------------------------------------------------------------
// k_init_prepare
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_init_prepare(const orbx_keypoint* __restrict__ kps,
                                                      const int32_t* __restrict__ m12,
                                                      const int32_t* __restrict__ counts,
                                                      const int32_t* __restrict__ draws,
                                                      const InitPair* __restrict__ descs, uint8_t* __restrict__ res,
                                                      InitLayout L)
{
    extern __shared__ float2 s_xy[];   // [cap] frame 1, [cap] frame 2
    __shared__ float s_norm[8];
    __shared__ int s_n;
    const InitPair d = descs[blockIdx.x];
    uint8_t* blk = res + (long long)blockIdx.x * L.stride;
    InitHdr* hdr = reinterpret_cast<InitHdr*>(blk);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n1 = max(0, min(d.cnt1 >= 0 ? counts[d.cnt1] : d.n1, L.cap));
    const int n2 = max(0, min(d.cnt2 >= 0 ? counts[d.cnt2] : d.n2, L.cap));
    const orbx_keypoint* k1 = kps + d.k1_off;
    const orbx_keypoint* k2 = kps + d.k2_off;
    float2* s1 = s_xy;
    float2* s2 = s_xy + L.cap;
    for (int i = tid; i < n1; i += blockDim.x) s1[i] = make_float2(k1[i].x, k1[i].y);
    for (int i = tid; i < n2; i += blockDim.x) s2[i] = make_float2(k2[i].x, k2[i].y);
    __syncthreads();

    if (wave == 0 && lane < 4) {
        // Normalize (src/Initializer.cc:747-793): the sums run over all
        // keypoints of the frame, sequentially in float
        const int axis = lane & 1, frame = lane >> 1;
        const float2* s = frame ? s2 : s1;
        const int n = frame ? n2 : n1;
        float mean = 0.f;
        for (int i = 0; i < n; i++) mean += axis ? s[i].y : s[i].x;
        mean = mean / (float)n;
        float dev = 0.f;
        for (int i = 0; i < n; i++) dev += fabsf((axis ? s[i].y : s[i].x) - mean);
        dev = dev / (float)n;
        const float sc = (float)(1.0 / (double)dev);
        s_norm[4 * frame + axis] = mean;
        s_norm[4 * frame + 2 + axis] = sc;
    } else if (wave == 1) {
        // mvMatches12 in i1 order (:54-63)
        const int32_t* m = m12 + d.m_off;
        int2* pairs = reinterpret_cast<int2*>(blk + L.o_pairs);
        float4* xy = reinterpret_cast<float4*>(blk + L.o_xy);
        const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
        int base = 0;
        for (int c = 0; c < n1; c += 64) {
            const int i = c + lane;
            int j = -1;
            if (i < n1) j = m[i];
            const bool ok = j >= 0 && j < n2;   // an index past frame 2 is not a match
            const unsigned long long bal = __ballot(ok);
            if (ok) {
                const int pos = base + __popcll(bal & lt_mask);   // < n1 <= cap
                pairs[pos] = make_int2(i, j);
                xy[pos] = make_float4(s1[i].x, s1[i].y, s2[j].x, s2[j].y);
            }
            base += __popcll(bal);
        }
        if (lane == 0) s_n = base;
    }
    __syncthreads();
    const int N = s_n;
    if (tid == 0) {
        hdr->n = N;
        hdr->best_h = -1;
        hdr->best_f = -1;
        hdr->pad0 = 0;
        hdr->pad1 = 0.f;
        for (int f = 0; f < 2; f++) {
            float* T = f ? hdr->T2 : hdr->T1;
            const float mx = s_norm[4 * f], my = s_norm[4 * f + 1], sx = s_norm[4 * f + 2], sy = s_norm[4 * f + 3];
            T[0] = sx;
            T[1] = 0.f;
            T[2] = -mx * sx;
            T[3] = 0.f;
            T[4] = sy;
            T[5] = -my * sy;
            T[6] = 0.f;
            T[7] = 0.f;
            T[8] = 1.f;
        }
        for (int i = 0; i < 8; i++) hdr->norm[i] = s_norm[i];
    }
    // mvSets (:80-95): vAvailableIndices is the identity but for the places
    // earlier picks of this iteration overwrote (at most 8), kept as a list
    int32_t* sets = reinterpret_cast<int32_t*>(blk + L.o_sets);
    const int M = min(d.max_iter, L.M);
    for (int it = tid; it < M; it += blockDim.x) {
        int pos[8], val[8];
        const int32_t* dr = draws + d.draw_off + (long long)it * 8;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            int idx = 0;
            if (N >= 8) {
                const int size = N - j;
                const int randi = (int)(((double)dr[j] / 2147483648.0) * (double)size);
                idx = randi;
                int back = size - 1;
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if (k < j) {
                        if (pos[k] == randi) idx = val[k];
                        if (pos[k] == size - 1) back = val[k];
                    }
                pos[j] = randi;
                val[j] = back;
            }
            sets[it * 8 + j] = idx;
        }
    }
}

// ---------------------------------------------------------------------------
// k_init_solve
// ---------------------------------------------------------------------------
// Fn = U diag(s1, s2, 0) V^T of the 3x3 Fpre: one-sided Jacobi on its columns
// (B V = U S), the column of the smallest norm dropped.
__device__ inline void rank2_3x3(const float* fpre, float* fn)
{
    const JacobiCols<3> m = hestenes(load_cols<3>(fpre));
    double nrm[3];
#pragma unroll
    for (int j = 0; j < 3; j++) nrm[j] = col_dot(m.a[j], m.a[j]);
    int kmin = 0;
    if (nrm[1] < nrm[kmin]) kmin = 1;
    if (nrm[2] < nrm[kmin]) kmin = 2;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++)
                if (k != kmin) acc += m.a[k][i] * m.v[k][j];
            fn[3 * i + j] = (float)acc;
        }
}

__global__ __launch_bounds__(256) void k_init_solve(const InitPair* __restrict__ descs, uint8_t* __restrict__ res,
                                                    InitLayout L)
{
    const InitPair d = descs[blockIdx.y];
    uint8_t* blk = res + (long long)blockIdx.y * L.stride;
    const InitHdr* hdr = reinterpret_cast<const InitHdr*>(blk);
    const int M = min(d.max_iter, L.M);
    const int N = hdr->n;
    const int r = threadIdx.x & 15;                                    // row of the hypothesis' matrices
    const int hyp = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;      // [0, M): H, [M, 2M): F
    const bool is_f = hyp >= M;
    const int it = is_f ? hyp - M : hyp;
    const bool active = hyp < 2 * M;
    float* Hn = reinterpret_cast<float*>(blk + L.o_Hn);
    float* Fn = reinterpret_cast<float*>(blk + L.o_Fn);
    float* H21 = reinterpret_cast<float*>(blk + L.o_H21);
    float* H12 = reinterpret_cast<float*>(blk + L.o_H12);
    float* F21 = reinterpret_cast<float*>(blk + L.o_F21);
    if (N < 8) {   // no sets (uniform over the workgroup): the taps read zero
        if (active && r < 9) {
            if (is_f) {
                Fn[it * 9 + r] = 0.f;
                F21[it * 9 + r] = 0.f;
            } else {
                Hn[it * 9 + r] = 0.f;
                H21[it * 9 + r] = 0.f;
                H12[it * 9 + r] = 0.f;
            }
        }
        return;
    }

    // row r of A (ComputeH21 :228-256: two rows per point; ComputeF21
    // :270-288: one, rows 8..15 zero) from float products, and row r of V = I
    double a[9], v[9];
#pragma unroll
    for (int j = 0; j < 9; j++) {
        a[j] = 0.0;
        v[j] = j == r ? 1.0 : 0.0;
    }
    if (active) {
        const int32_t* set = reinterpret_cast<const int32_t*>(blk + L.o_sets) + it * 8;
        const float4* xy = reinterpret_cast<const float4*>(blk + L.o_xy);
        const int pt = is_f ? r : (r >> 1);
        if (pt < 8) {
            const int idx = min(max(set[pt], 0), N - 1);
            const float4 p = xy[idx];
            // vPn = (pt - mean) * s (:769-785)
            const float u1 = (p.x - hdr->norm[0]) * hdr->norm[2];
            const float v1 = (p.y - hdr->norm[1]) * hdr->norm[3];
            const float u2 = (p.z - hdr->norm[4]) * hdr->norm[6];
            const float v2 = (p.w - hdr->norm[5]) * hdr->norm[7];
            if (is_f) {
                a[0] = (double)(u2 * u1);
                a[1] = (double)(u2 * v1);
                a[2] = (double)u2;
                a[3] = (double)(v2 * u1);
                a[4] = (double)(v2 * v1);
                a[5] = (double)v2;
                a[6] = (double)u1;
                a[7] = (double)v1;
                a[8] = 1.0;
            } else if ((r & 1) == 0) {
                a[3] = (double)(-u1);
                a[4] = (double)(-v1);
                a[5] = -1.0;
                a[6] = (double)(v2 * u1);
                a[7] = (double)(v2 * v1);
                a[8] = (double)v2;
            } else {
                a[0] = (double)u1;
                a[1] = (double)v1;
                a[2] = 1.0;
                a[6] = (double)(-u2 * u1);
                a[7] = (double)(-u2 * v1);
                a[8] = (double)(-u2);
            }
        }
    }

    // One-sided Jacobi on the columns of A.  The butterfly sums are the same
    // bits in all 16 lanes, so a row takes its branches together; the sweep
    // loop is uniform over the wave (the cross-lane reads stay convergent).
    double floor = 0.0;
#pragma unroll
    for (int j = 0; j < 9; j++) floor += a[j] * a[j];
    floor = row_sum16(floor) * kInitFloor;
    for (int sweep = 0; sweep < kInitSweeps; sweep++) {
        bool rot = false;
#pragma unroll
        for (int p = 0; p < 8; p++)
#pragma unroll
            for (int q = p + 1; q < 9; q++) {
                const double al = row_sum16(a[p] * a[p]);
                const double be = row_sum16(a[q] * a[q]);
                const double ga = row_sum16(a[p] * a[q]);
                if (jacobi_wants(al, be, ga, floor)) {
                    rot = true;
                    const JacobiRot g = jacobi_cs(al, be, ga);
                    const double ap = a[p], aq = a[q];
                    a[p] = g.c * ap - g.s * aq;
                    a[q] = g.s * ap + g.c * aq;
                    const double vp = v[p], vq = v[q];
                    v[p] = g.c * vp - g.s * vq;
                    v[q] = g.s * vp + g.c * vq;
                }
            }
        if (!__any(rot)) break;
    }
    // the null vector: V's column of the smallest column norm of A V
    double best = row_sum16(a[0] * a[0]);
    double nv = v[0];
#pragma unroll
    for (int j = 1; j < 9; j++) {
        const double nj = row_sum16(a[j] * a[j]);
        if (nj < best) {
            best = nj;
            nv = v[j];
        }
    }
    // every lane of the row gathers the 3x3 (entry k sits in lane k)
    const float mine = (float)nv;
    float x[9];
    const int row_base = (threadIdx.x & 63) & ~15;
#pragma unroll
    for (int k = 0; k < 9; k++) x[k] = __shfl(mine, row_base + k);
    if (!active || r != 0) return;

    if (is_f) {
        float fn[9], T2t[9], tmp[9], out[9];
        rank2_3x3(x, fn);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) T2t[3 * i + j] = hdr->T2[3 * j + i];
        mul3(T2t, fn, tmp);          // F21i = T2t * Fn * T1 (:210), left product first
        mul3(tmp, hdr->T1, out);
#pragma unroll
        for (int k = 0; k < 9; k++) {
            Fn[it * 9 + k] = fn[k];
            F21[it * 9 + k] = out[k];
        }
    } else {
        float T2inv[9], tmp[9], h21[9], h12[9];
        inv3(hdr->T2, T2inv);        // T2.inv() (:132)
        mul3(T2inv, x, tmp);         // H21i = T2inv * Hn * T1 (:158)
        mul3(tmp, hdr->T1, h21);
        inv3(h21, h12);              // H12i = H21i.inv() (:159)
#pragma unroll
        for (int k = 0; k < 9; k++) {
            Hn[it * 9 + k] = x[k];
            H21[it * 9 + k] = h21[k];
            H12[it * 9 + k] = h12[k];
        }
    }
}

// ---------------------------------------------------------------------------
// k_init_score
// ---------------------------------------------------------------------------
// chiSquare1 / chiSquare2 of CheckHomography (:350-372) for one match.
__device__ inline void h_chi(const float* h, const float* hi, float4 p, float inv_s2, float& chi1, float& chi2)
{
    const float u1 = p.x, v1 = p.y, u2 = p.z, v2 = p.w;
    const float w2in1inv = (float)(1.0 / (double)(hi[6] * u2 + hi[7] * v2 + hi[8]));
    const float u2in1 = (hi[0] * u2 + hi[1] * v2 + hi[2]) * w2in1inv;
    const float v2in1 = (hi[3] * u2 + hi[4] * v2 + hi[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    chi1 = squareDist1 * inv_s2;
    const float w1in2inv = (float)(1.0 / (double)(h[6] * u1 + h[7] * v1 + h[8]));
    const float u1in2 = (h[0] * u1 + h[1] * v1 + h[2]) * w1in2inv;
    const float v1in2 = (h[3] * u1 + h[4] * v1 + h[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    chi2 = squareDist2 * inv_s2;
}

// chiSquare1 / chiSquare2 of CheckFundamental (:426-452).
__device__ inline void f_chi(const float* f, float4 p, float inv_s2, float& chi1, float& chi2)
{
    const float u1 = p.x, v1 = p.y, u2 = p.z, v2 = p.w;
    const float a2 = f[0] * u1 + f[1] * v1 + f[2];
    const float b2 = f[3] * u1 + f[4] * v1 + f[5];
    const float c2 = f[6] * u1 + f[7] * v1 + f[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    chi1 = squareDist1 * inv_s2;
    const float a1 = f[0] * u2 + f[3] * v2 + f[6];
    const float b1 = f[1] * u2 + f[4] * v2 + f[7];
    const float c1 = f[2] * u2 + f[5] * v2 + f[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    chi2 = squareDist2 * inv_s2;
}

__global__ __launch_bounds__(1024) void k_init_score(const InitPair* __restrict__ descs, uint8_t* __restrict__ res,
                                                     InitLayout L)
{
    extern __shared__ float4 s_m[];   // [cap] compacted (u1, v1, u2, v2)
    __shared__ float s_score[2 * kInitMaxIter];
    __shared__ int s_best[2];
    __shared__ float s_bs[2];
    const InitPair d = descs[blockIdx.x];
    uint8_t* blk = res + (long long)blockIdx.x * L.stride;
    InitHdr* hdr = reinterpret_cast<InitHdr*>(blk);
    const int M = min(d.max_iter, L.M);
    const int N = min(hdr->n, L.cap);
    const int tid = threadIdx.x;
    const float4* xy = reinterpret_cast<const float4*>(blk + L.o_xy);
    const float* H21 = reinterpret_cast<const float*>(blk + L.o_H21);
    const float* H12 = reinterpret_cast<const float*>(blk + L.o_H12);
    const float* F21 = reinterpret_cast<const float*>(blk + L.o_F21);
    float* score_h = reinterpret_cast<float*>(blk + L.o_sh);
    float* score_f = reinterpret_cast<float*>(blk + L.o_sf);
    uint8_t* inl_h = blk + L.o_inh;
    uint8_t* inl_f = blk + L.o_inf;
    for (int i = tid; i < N; i += blockDim.x) s_m[i] = xy[i];
    __syncthreads();

    const float th_h = 5.991f, th_f = 3.841f, th_score = 5.991f;
    const float inv_s2 = (float)(1.0 / (double)(d.sigma * d.sigma));
    const bool solved = hdr->n >= 8;
    for (int t = tid; t < 2 * M; t += blockDim.x) {
        const bool is_f = t >= M;
        const int it = is_f ? t - M : t;
        float score = 0.f;
        if (solved) {
            float m[9], mi[9];
#pragma unroll
            for (int k = 0; k < 9; k++) {
                m[k] = is_f ? F21[it * 9 + k] : H21[it * 9 + k];
                mi[k] = is_f ? 0.f : H12[it * 9 + k];
            }
            if (is_f) {
                for (int i = 0; i < N; i++) {
                    float c1, c2;
                    f_chi(m, s_m[i], inv_s2, c1, c2);
                    if (!(c1 > th_f)) score += th_score - c1;
                    if (!(c2 > th_f)) score += th_score - c2;
                }
            } else {
                for (int i = 0; i < N; i++) {
                    float c1, c2;
                    h_chi(m, mi, s_m[i], inv_s2, c1, c2);
                    if (!(c1 > th_h)) score += th_h - c1;
                    if (!(c2 > th_h)) score += th_h - c2;
                }
            }
        }
        s_score[t] = score;
        (is_f ? score_f : score_h)[it] = score;
    }
    __syncthreads();
    // the first iteration whose score exceeds every earlier best (:163, :214)
    // (threads 0 and 1: a workgroup of few iterations has one wave only)
    if (tid < 2) {
        const int model = tid;
        float bs = 0.f;
        int best = -1;
        for (int it = 0; it < M; it++)
            if (s_score[model * M + it] > bs) {
                bs = s_score[model * M + it];
                best = it;
            }
        s_best[model] = best;
        s_bs[model] = bs;
    }
    __syncthreads();
    const int bh = s_best[0], bf = s_best[1];
    if (tid == 0) {
        hdr->best_h = bh;
        hdr->best_f = bf;
        hdr->SH = s_bs[0];
        hdr->SF = s_bs[1];
        hdr->RH = s_bs[0] / (s_bs[0] + s_bs[1]);
        for (int k = 0; k < 9; k++) {
            hdr->H21[k] = bh >= 0 ? H21[bh * 9 + k] : 0.f;
            hdr->F21[k] = bf >= 0 ? F21[bf * 9 + k] : 0.f;
        }
    }
    // vbMatchesInliers of the two winners, recomputed
    float h[9], hi[9], f[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        h[k] = bh >= 0 ? H21[bh * 9 + k] : 0.f;
        hi[k] = bh >= 0 ? H12[bh * 9 + k] : 0.f;
        f[k] = bf >= 0 ? F21[bf * 9 + k] : 0.f;
    }
    for (int i = tid; i < N; i += blockDim.x) {
        float c1, c2;
        uint8_t in_h = 0, in_f = 0;
        if (bh >= 0) {
            h_chi(h, hi, s_m[i], inv_s2, c1, c2);
            in_h = !(c1 > th_h) && !(c2 > th_h);
        }
        if (bf >= 0) {
            f_chi(f, s_m[i], inv_s2, c1, c2);
            in_f = !(c1 > th_f) && !(c2 > th_f);
        }
        inl_h[i] = in_h;
        inl_f[i] = in_f;
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {

int launch_init(orbx_ctx* ctx, int P, const orbx_keypoint* kps, const int32_t* m12, const int32_t* counts,
                const int32_t* draws, const InitPair* descs, uint8_t* res, const InitLayout& L)
{
    hipStream_t st = ctx->stream;
    timer_begin(ctx, "init");
    timer_begin(ctx, "init.prepare");
    hipLaunchKernelGGL(k_init_prepare, dim3(P), dim3(256), (size_t)L.cap * 2 * sizeof(float2), st, kps, m12, counts,
                       draws, descs, res, L);
    timer_end(ctx, "init.prepare");
    ORBX_HIP_CHECK(hipGetLastError());
    timer_begin(ctx, "init.solve");
    hipLaunchKernelGGL(k_init_solve, dim3((2 * L.M * 16 + 255) / 256, P), dim3(256), 0, st, descs, res, L);
    timer_end(ctx, "init.solve");
    ORBX_HIP_CHECK(hipGetLastError());
    const int threads = std::min(1024, (2 * L.M + 63) / 64 * 64);
    timer_begin(ctx, "init.score");
    hipLaunchKernelGGL(k_init_score, dim3(P), dim3(threads), (size_t)L.cap * sizeof(float4), st, descs, res, L);
    timer_end(ctx, "init.score");
    timer_end(ctx, "init");
    ORBX_HIP_CHECK(hipGetLastError());
    return ORBX_OK;
}

int check_common(float sigma, int max_iter, const int32_t* draws, long long n_draws)
{
    if (!(sigma > 0.f) || max_iter < 1 || max_iter > kInitMaxIter || !draws) return ORBX_ERR_ARG;
    for (long long i = 0; i < n_draws; i++)
        if (draws[i] < 0) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// One pair's result block (host copy) into the query's outputs and taps.
void scatter(const uint8_t* blk, const InitLayout& L, int M, orbx_init_query* q)
{
    const InitHdr* h = reinterpret_cast<const InitHdr*>(blk);
    const int N = h->n;
    q->n_matches = N;
    q->best_h = h->best_h;
    q->best_f = h->best_f;
    q->SH = h->SH;
    q->SF = h->SF;
    q->RH = h->RH;
    if (h->best_h >= 0) std::memcpy(q->H21, h->H21, sizeof(q->H21));
    if (h->best_f >= 0) std::memcpy(q->F21, h->F21, sizeof(q->F21));
    const int n = std::min(N, std::min(q->cap, L.cap));
    if (q->inliers_h && n > 0) std::memcpy(q->inliers_h, blk + L.o_inh, n);
    if (q->inliers_f && n > 0) std::memcpy(q->inliers_f, blk + L.o_inf, n);
    auto tap = [&](void* dst, int off, size_t bytes) {
        if (dst) std::memcpy(dst, blk + off, bytes);
    };
    tap(q->sets, L.o_sets, (size_t)M * 32);
    tap(q->Hn, L.o_Hn, (size_t)M * 36);
    tap(q->Fn, L.o_Fn, (size_t)M * 36);
    tap(q->H21_all, L.o_H21, (size_t)M * 36);
    tap(q->H12_all, L.o_H12, (size_t)M * 36);
    tap(q->F21_all, L.o_F21, (size_t)M * 36);
    tap(q->score_h, L.o_sh, (size_t)M * 4);
    tap(q->score_f, L.o_sf, (size_t)M * 4);
    if (q->T1) std::memcpy(q->T1, h->T1, 36);
    if (q->T2) std::memcpy(q->T2, h->T2, 36);
}

}  // namespace
}  // namespace orbx

using namespace orbx;

extern "C" int orbx_init_models_batch(orbx_ctx* ctx, int B, orbx_init_query* qs)
{
    if (!ctx || !qs || B < 1) return ORBX_ERR_ARG;
    // argument rules, before any device work
    int Mmax = 0, cap = 1;
    long long n_kp = 0, n_m = 0, n_dr = 0;
    for (int b = 0; b < B; b++) {
        const orbx_init_query& q = qs[b];
        if (q.n1 < 0 || q.n2 < 0 || (q.n1 > 0 && (!q.keys1 || !q.matches12)) || (q.n2 > 0 && !q.keys2))
            return ORBX_ERR_ARG;
        const int r = check_common(q.sigma, q.max_iter, q.draws, (long long)std::max(q.max_iter, 0) * 8);
        if (r != ORBX_OK) return r;
        if (q.n1 > kMaxFeatures || q.n2 > kMaxFeatures) return ORBX_ERR_UNSUPPORTED;
        int N = 0;
        for (int i = 0; i < q.n1; i++) {
            if (q.matches12[i] >= q.n2) return ORBX_ERR_ARG;   // the reference would index past mvKeys2
            N += q.matches12[i] >= 0;
        }
        if (q.cap < N) return ORBX_ERR_CAPACITY;
        Mmax = std::max(Mmax, q.max_iter);
        cap = std::max(cap, std::max(q.n1, q.n2));
        n_kp += q.n1 + q.n2;
        n_m += q.n1;
        n_dr += (long long)q.max_iter * 8;
    }
    ctx_enter(ctx);
    const InitLayout L = make_layout(Mmax, cap);
    // one upload: descriptors | keypoints | matches | draws (each array the queries' end to end)
    PackedStage st(ctx);
    const Region<InitPair> descs = st.take<InitPair>(B);
    const Region<orbx_keypoint> kps = st.take<orbx_keypoint>(n_kp);
    const Region<int32_t> m12 = st.take<int32_t>(n_m), draws = st.take<int32_t>(n_dr);
    int r = st.open((size_t)B * L.stride);
    if (r != ORBX_OK) return r;
    long long kp = 0, mm = 0, dr = 0;
    for (int b = 0; b < B; b++) {
        const orbx_init_query& q = qs[b];
        InitPair& d = st.host(descs)[b];
        d.k1_off = kp;
        d.k2_off = kp + q.n1;
        d.m_off = mm;
        d.draw_off = dr;
        d.n1 = q.n1;
        d.n2 = q.n2;
        d.cnt1 = d.cnt2 = -1;
        d.max_iter = q.max_iter;
        d.sigma = q.sigma;
        if (q.n1) std::memcpy(st.host(kps) + kp, q.keys1, (size_t)q.n1 * sizeof(orbx_keypoint));
        if (q.n2) std::memcpy(st.host(kps) + kp + q.n1, q.keys2, (size_t)q.n2 * sizeof(orbx_keypoint));
        if (q.n1) std::memcpy(st.host(m12) + mm, q.matches12, (size_t)q.n1 * 4);
        std::memcpy(st.host(draws) + dr, q.draws, (size_t)q.max_iter * 32);
        kp += q.n1 + q.n2;
        mm += q.n1;
        dr += (long long)q.max_iter * 8;
    }
    ResultBlocks res(ctx, st.behind(), B, L.stride);
    if ((r = st.upload()) != ORBX_OK) return r;
    if ((r = launch_init(ctx, B, st.dev(kps), st.dev(m12), nullptr, st.dev(draws), st.dev(descs), res.dev, L)) != ORBX_OK)
        return r;
    if ((r = res.read()) != ORBX_OK) return r;
    for (int b = 0; b < B; b++) scatter(res.block(b), L, qs[b].max_iter, &qs[b]);
    return ORBX_OK;
}

extern "C" int orbx_init_models(orbx_ctx* ctx, orbx_init_query* q) { return orbx_init_models_batch(ctx, 1, q); }

extern "C" int orbx_dev_init_models(orbx_ctx* ctx, int first, int count, int seq_len, float sigma, int max_iter,
                                    const int32_t* draws)
{
    if (!ctx || first < 0 || count < 1 || first + count > ctx->slots || seq_len < 1) return ORBX_ERR_ARG;
    int r = check_common(sigma, max_iter, draws, (long long)count * std::max(max_iter, 0) * 8);
    if (r != ORBX_OK) return r;
    const int nf = ctx->geom.nfeatures;
    if (nf > kMaxFeatures) return ORBX_ERR_UNSUPPORTED;
    ctx_enter(ctx);   // orders the context stream after a pending asynchronous match
    std::vector<InitPair> descs;
    std::vector<int> pair_of(count, -1);
    for (int k = 0; k < count; k++) {
        const int s = first + k;
        if (s % seq_len == 0) continue;
        InitPair d;
        d.k1_off = (long long)(s - 1) * nf;
        d.k2_off = (long long)s * nf;
        d.m_off = (long long)s * nf;
        d.draw_off = (long long)k * max_iter * 8;
        d.n1 = d.n2 = 0;
        d.cnt1 = s - 1;
        d.cnt2 = s;
        d.max_iter = max_iter;
        d.sigma = sigma;
        pair_of[k] = (int)descs.size();
        descs.push_back(d);
    }
    const int P = (int)descs.size();
    const InitLayout L = make_layout(max_iter, std::max(nf, 1));
    ctx->init_count = 0;
    ctx->rec_count = 0;   // a reconstruction belongs to the models run it read
    if ((size_t)P * L.stride > ctx->init_res_bytes) {
        if (ctx->init_res) (void)hipFree(ctx->init_res);
        ctx->init_res = nullptr;
        ctx->init_res_bytes = 0;
        if (hipMalloc(&ctx->init_res, (size_t)P * L.stride) != hipSuccess) return ORBX_ERR_NOMEM;
        ctx->init_res_bytes = (size_t)P * L.stride;
    }
    if (P > 0) {
        PackedStage st(ctx);
        const Region<InitPair> pairs = st.take(P, descs.data());
        const Region<int32_t> dr = st.take((size_t)count * max_iter * 8, draws);
        if ((r = st.open(0)) != ORBX_OK || (r = st.upload()) != ORBX_OK) return r;
        // the blob is freed on return: the copy is waited for, the kernels are not
        ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        r = launch_init(ctx, P, ctx->out_kps, ctx->match12, ctx->out_n, st.dev(dr), st.dev(pairs),
                        static_cast<uint8_t*>(ctx->init_res), L);
        if (r != ORBX_OK) return r;
    }
    ctx->init_first = first;
    ctx->init_count = count;
    ctx->init_iter = max_iter;
    ctx->init_sigma = sigma;
    ctx->init_pair = pair_of;
    return ORBX_OK;
}

extern "C" int orbx_dev_read_init_models(orbx_ctx* ctx, int slot, orbx_init_query* out)
{
    if (!ctx || !out || ctx->init_count == 0 || slot < ctx->init_first || slot >= ctx->init_first + ctx->init_count)
        return ORBX_ERR_ARG;
    const int p = ctx->init_pair[slot - ctx->init_first];
    if (p < 0) return ORBX_ERR_ARG;   // a sequence start has no pair
    ctx_enter(ctx);
    const int M = ctx->init_iter;
    const InitLayout L = make_layout(M, std::max(ctx->geom.nfeatures, 1));
    ResultBlocks blk(ctx, static_cast<uint8_t*>(ctx->init_res) + (size_t)p * L.stride, 1, L.stride);
    const int r = blk.read();
    if (r != ORBX_OK) return r;
    const int N = reinterpret_cast<const InitHdr*>(blk.block(0))->n;
    out->n_matches = N;
    if (out->cap < N) return ORBX_ERR_CAPACITY;
    scatter(blk.block(0), L, M, out);
    return ORBX_OK;
}
