// Optimizer::OptimizeSim3 on MI355X (FP64): the Sim3 refinement of
// LoopClosing::ComputeSim3 (src/Optimizer.cc:791-987) for batches of
// loop-closure candidates.
//
// g2o subset (as the reference configures it): one free VertexSim3Expmap
// against fixed points through an EdgeSim3ProjectXYZ (e12) and an
// EdgeInverseSim3ProjectXYZ (e21) per correspondence, Huber, BlockSolverX +
// LinearSolverDense (Eigen LDLT, diagonal pivoting, 7 x 7) and
// OptimizationAlgorithmLevenberg with ORB-SLAM's stop rule.  Both edge
// classes leave linearizeOplus to BaseBinaryEdge: central differences with
// delta = 1e-9 on the Sim3 vertex (base_binary_edge.hpp:131-205).
//
// Mapping: one workgroup per candidate -- a wavefront in a batch, four
// wavefronts for a lone call -- and both optimize() rounds with their checks
// in ONE launch.  A thread handles both edges of a correspondence; the
// correspondences (camera-frame points, observations, the two information
// values, a flag) live in the candidate's block of global memory, written by
// the kernel's own set-up pass and re-read by every pass, so no edge count is
// bounded by LDS.  Per LM iteration the 15 estimates of the linearisation
// (the current one and Sim3(+-delta e_d) * S for the 7 dimensions) and their
// inverses are computed once, a lane each, into LDS; every thread then
// evaluates the 15 projections of each of its two edges, forms the numeric
// Jacobians and writes the pair's 72 terms (per edge the robust chi2, the 28
// lower entries of B^T W B and the 7 of B^T omega_r) to an LDS row; lane q of
// the first wavefront adds column q over the rows in g2o's edge order
// e12_0, e21_0, e12_1, ... -- every sum is the sequential sum of the
// restatement (tests/sim3opt_numpy.py).  A trial is one error pass summed the
// same way.  The sums reach every thread through LDS, so the LDLT, the
// exp-map update and the accept / reject logic run redundantly on uniform
// data.  A removed pair writes +0.0 terms: the sums start at +0.0 and
// round-to-nearest never makes -0.0 of them, so that leaves every bit as
// skipping the pair would.
//
// Stored-error semantics: the checks read each edge's _error as left by the
// LAST computeActiveErrors -- the final trial's state even when that trial was
// rejected.  The kernel keeps that estimate ("errest", orbx_pose.hip's
// errpose) and evaluates the tested chi2 there.
//
// The Jacobian path needs Sim3(update) at +-1e-9 e_d only: the |sigma| < eps,
// theta < eps branch, + - * /, sqrt and exp at 0 and +-1e-9.  The two
// exponentials are constants (the correctly rounded values), so the whole
// linearisation is reproducible bit for bit; the device's exp / sin / cos
// enter in the LM update alone.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "orbx_device.h"
#include "orbx_internal.h"
#include "orbx_lm.h"
#include "orbx_match_common.h"
#include "orbx_se3.h"
#include "orbx_sim3_dev.h"
#include "orbx_stage.h"

namespace orbx {

constexpr int kSoLm = ORBX_SIM3_OPT_MAX_LM;
constexpr int kSoTrials = ORBX_SIM3_OPT_MAX_TRIALS;
constexpr int kSoWide = 4;          // wavefronts of a lone call's workgroup
constexpr int kSoTerms = 36;        // per edge: chi2, 28 of H, 7 of b
constexpr int kSoStride = 73;       // doubles per LDS row (72 terms + 1: odd, so rows spread over the banks)
static_assert(64 * kSoWide * kSoStride * sizeof(double) <= 150 * 1024, "the term rows of a lone call fit gfx950's LDS");

// One candidate: device pointers to its inputs.
struct Sim3OptProb {
    const orbx_keypoint* k1;
    const orbx_keypoint* k2;
    const int32_t* ci;       // n: KF1 keypoint of each correspondence (vnIndexEdge)
    const int32_t* cj;       // n: KF2 keypoint
    const float* pos1;
    const float* pos2;
    const float* isig1;      // KF1's mvInvLevelSigma2
    const float* sig2;       // KF2's mvLevelSigma2
    int32_t n, nlevels, taps, pad;
    float T1w[12], T2w[12];  // rows 0..2 of Tcw
    float cam1[4], cam2[4];
    float R12[9], t12[3], s12, th2;
    double delta;            // (double) sqrtf(th2)
};

struct Sim3OptIter {
    double est[8], chi2, H[28], b[7], lambda, dx[kSoTrials][7];
    int32_t trials, pad;
};

struct Sim3OptHdr {
    double est[8], check_est[2][8];
    float R12[9], t12[3], s12, padf[3];
    int32_t n_in, n_bad, early, n_lm;
    int32_t iters[2], trials[2], npd[2], pad[2];
};

// Byte offsets inside one candidate's block.
struct Sim3OptLayout {
    long long stride;
    int o_x1, o_x2, o_obs, o_w, o_flag, o_it, o_err, o_J, o_chi;
    int cap;
};

inline Sim3OptLayout sim3opt_layout(int cap, bool taps)
{
    Sim3OptLayout L;
    BlockOffsets o;
    o.take(sizeof(Sim3OptHdr));
    L.o_x1 = o.take((long long)cap * 12);
    L.o_x2 = o.take((long long)cap * 12);
    L.o_obs = o.take((long long)cap * 16);
    L.o_w = o.take((long long)cap * 8);
    L.o_flag = o.take(cap);
    L.o_it = o.take(taps ? (long long)kSoLm * sizeof(Sim3OptIter) : 0);
    L.o_err = o.take(taps ? (long long)cap * 32 : 0);
    L.o_J = o.take(taps ? (long long)cap * 224 : 0);
    L.o_chi = o.take(taps ? (long long)cap * 32 : 0);
    L.stride = o.end;
    L.cap = cap;
    return L;
}

// obs - cam_map(project(S.map(X))) (types_seven_dof_expmap.h:138-167)
__device__ inline void sim3_edge_error(const double* S, const double X[3], double o0, double o1, const CamD& c,
                                       double& e0, double& e1)
{
    const Q q{S[0], S[1], S[2], S[3]};
    double r[3];
    qrot(q, X, r);
    const double s = S[7];
    const double x = s * r[0] + S[4], y = s * r[1] + S[5], z = s * r[2] + S[6];
    e0 = o0 - (x / z * c.fx + c.cx);
    e1 = o1 - (y / z * c.fy + c.cy);
}

// One edge's 36 terms at the 15 estimates S[0..14] (LDS): computeError, the
// central differences of BaseBinaryEdge::linearizeOplus, robustify and
// constructQuadraticForm's products for the Sim3 vertex
// (base_binary_edge.hpp:91-113), written to row[0, 36).
__device__ inline void so_edge_terms(const double (*S)[8], const double X[3], double o0, double o1, const CamD& cam,
                                     double info, double delta, double* row, bool tap, double* tap_err, double* tap_J)
{
    constexpr double scalar = 1.0 / (2 * kSoDelta);
    double er0, er1, J0[7], J1[7];
    sim3_edge_error(S[0], X, o0, o1, cam, er0, er1);
#pragma unroll
    for (int d = 0; d < 7; d++) {
        double p0, p1, m0, m1;
        sim3_edge_error(S[1 + 2 * d], X, o0, o1, cam, p0, p1);
        sim3_edge_error(S[2 + 2 * d], X, o0, o1, cam, m0, m1);
        J0[d] = scalar * (p0 - m0);
        J1[d] = scalar * (p1 - m1);
    }
    if (tap) {
        tap_err[0] = er0;
        tap_err[1] = er1;
#pragma unroll
        for (int d = 0; d < 7; d++) {
            tap_J[d] = J0[d];
            tap_J[7 + d] = J1[d];
        }
    }
    double rho0, rho1;
    huber(er0 * (info * er0) + er1 * (info * er1), delta, rho0, rho1);
    row[0] = rho0;
    const double w = rho1 * info;
    const double om0 = -(info * er0) * rho1, om1 = -(info * er1) * rho1;
    int k = 1;
#pragma unroll
    for (int i = 0; i < 7; i++)
#pragma unroll
        for (int j = 0; j <= i; j++, k++) row[k] = (J0[i] * w) * J0[j] + (J1[i] * w) * J1[j];
#pragma unroll
    for (int i = 0; i < 7; i++) row[29 + i] = J0[i] * om0 + J1[i] * om1;
}

template <int kW>
__global__ __launch_bounds__(64 * kW) void k_sim3_opt(const Sim3OptProb* __restrict__ probs, uint8_t* __restrict__ res,
                                                      Sim3OptLayout L)
{
    constexpr int kT = 64 * kW;
    __shared__ double s_rows[kT * kSoStride];
    __shared__ double s_est[15][8], s_inv[15][8];
    __shared__ double s_sum[kSoTerms];
    __shared__ int s_cnt[2];
    const Sim3OptProb& P = probs[blockIdx.x];
    uint8_t* blk = res + (long long)blockIdx.x * L.stride;
    Sim3OptHdr* hdr = reinterpret_cast<Sim3OptHdr*>(blk);
    const int tid = threadIdx.x;
    const int n = max(0, min(P.n, L.cap));
    const bool taps = P.taps != 0;
    float* gx1 = reinterpret_cast<float*>(blk + L.o_x1);
    float* gx2 = reinterpret_cast<float*>(blk + L.o_x2);
    float* gobs = reinterpret_cast<float*>(blk + L.o_obs);
    float* gw = reinterpret_cast<float*>(blk + L.o_w);
    uint8_t* gflag = blk + L.o_flag;
    Sim3OptIter* tap_it = reinterpret_cast<Sim3OptIter*>(blk + L.o_it);
    double* tap_err = reinterpret_cast<double*>(blk + L.o_err);
    double* tap_J = reinterpret_cast<double*>(blk + L.o_J);
    double* tap_chi = reinterpret_cast<double*>(blk + L.o_chi);
    const CamD cam1{(double)P.cam1[0], (double)P.cam1[1], (double)P.cam1[2], (double)P.cam1[3]};
    const CamD cam2{(double)P.cam2[0], (double)P.cam2[1], (double)P.cam2[2], (double)P.cam2[3]};
    const double delta = P.delta;
    const double th2 = (double)P.th2;

    // the correspondences (:844-923): P3D1c = R1w * P3D1w + t1w in the float
    // gemm of the Sim3 solver (FP64 accumulation over k in order, the addend,
    // rounded once), the observations and the two information values
#pragma unroll 1
    for (int c = tid; c < n; c += kT) {
        const int i1 = P.ci[c], i2 = P.cj[c];
        const orbx_keypoint ka = P.k1[i1], kb = P.k2[i2];
        const float* a = P.pos1 + 3 * (long long)i1;
        const float* b = P.pos2 + 3 * (long long)i2;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            double acc = (double)P.T1w[4 * r] * (double)a[0];
            acc = acc + (double)P.T1w[4 * r + 1] * (double)a[1];
            acc = acc + (double)P.T1w[4 * r + 2] * (double)a[2];
            gx1[3 * c + r] = (float)(acc + (double)P.T1w[4 * r + 3]);
            acc = (double)P.T2w[4 * r] * (double)b[0];
            acc = acc + (double)P.T2w[4 * r + 1] * (double)b[1];
            acc = acc + (double)P.T2w[4 * r + 2] * (double)b[2];
            gx2[3 * c + r] = (float)(acc + (double)P.T2w[4 * r + 3]);
        }
        gobs[4 * c] = ka.x;
        gobs[4 * c + 1] = ka.y;
        gobs[4 * c + 2] = kb.x;
        gobs[4 * c + 3] = kb.y;
        gw[2 * c] = P.isig1[min(max(ka.octave, 0), P.nlevels - 1)];
        gw[2 * c + 1] = P.sig2[min(max(kb.octave, 0), P.nlevels - 1)];   // GetSigma2, not its inverse (:912)
        gflag[c] = 0;
    }
    __syncthreads();

    // vertex 0: Sim3(toMatrix3d(R), toVector3d(t), s) -- widened floats, Eigen's
    // quaternion of the matrix, no normalisation
    double est[8], errest[8];
    {
        double R[9];
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = (double)P.R12[i];
        const Q q = qfrom(R);
        est[0] = q.x; est[1] = q.y; est[2] = q.z; est[3] = q.w;
#pragma unroll
        for (int i = 0; i < 3; i++) est[4 + i] = (double)P.t12[i];
        est[7] = (double)P.s12;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) errest[i] = est[i];

    // a pair's inputs
    auto load_pair = [&](int c, double X1[3], double X2[3], double o[4], double w[2]) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
            X1[r] = (double)gx1[3 * c + r];
            X2[r] = (double)gx2[3 * c + r];
        }
#pragma unroll
        for (int r = 0; r < 4; r++) o[r] = (double)gobs[4 * c + r];
        w[0] = (double)gw[2 * c];
        w[1] = (double)gw[2 * c + 1];
    };
    // Q sequential sums over the rows of the groups of kT pairs: fill(c, row)
    // writes pair c's 2 x Q terms to row[0, Q) and row[36, 36 + Q); lane q < Q
    // of wave 0 adds both per row in pair order.  The results land in
    // s_sum[0, Q) for every thread.
    auto seq_sums = [&](auto Qc, auto&& fill) {
        constexpr int Qn = decltype(Qc)::value;
        double acc = 0.0;
#pragma unroll 1
        for (int g = 0; g < n; g += kT) {
            const int cnt = min(kT, n - g);
            const int rows8 = (cnt + 7) & ~7;   // the chain runs in blocks of 8 rows
            if (tid < rows8) {
                double* row = s_rows + tid * kSoStride;
                const int c = g + tid;
                if (c < n && gflag[c] == 0) {
                    fill(c, row);
                } else {
                    asm volatile("" ::: "memory");   // keeps the zero stores a branch of their own
#pragma unroll
                    for (int q = 0; q < Qn; q++) {
                        row[q] = 0.0;
                        row[kSoTerms + q] = 0.0;
                    }
                }
            }
            __syncthreads();
            if (tid < Qn) {
#pragma unroll 1
                for (int k0 = 0; k0 < rows8; k0 += 8) {
                    double v[16];
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        v[2 * j] = s_rows[(k0 + j) * kSoStride + tid];
                        v[2 * j + 1] = s_rows[(k0 + j) * kSoStride + kSoTerms + tid];
                    }
#pragma unroll
                    for (int j = 0; j < 16; j++) acc += v[j];
                }
            }
            __syncthreads();
        }
        if (tid < Qn) s_sum[tid] = acc;
        __syncthreads();
    };

    int n_bad = 0, n_in = 0, early = 0, n_lm = 0;
    if (tid == 0) {
#pragma unroll
        for (int r = 0; r < 2; r++) hdr->iters[r] = hdr->trials[r] = hdr->npd[r] = 0;
    }
#pragma unroll 1
    for (int round = 0; round < 2 && n > 0; round++) {
        const int its = round == 0 ? 5 : (n_bad > 0 ? 10 : 5);   // nMoreIterations (:951-955)
        LmState lm{0, 2, 0};
        int iters = 0, trials = 0, npd = 0;
#pragma unroll 1
        for (int iter = 0; iter < its; iter++) {
            // the 15 estimates of the linearisation and their inverses, a lane each
            if (tid < 15) {
                double pe[8], pi[8];
                if (tid == 0) {
#pragma unroll
                    for (int i = 0; i < 8; i++) pe[i] = est[i];
                } else {
                    const int d = (tid - 1) >> 1;
                    const bool minus = ((tid - 1) & 1) != 0;
                    const double v = minus ? -kSoDelta : kSoDelta;
                    double u[7], ex[8];
#pragma unroll
                    for (int k = 0; k < 7; k++) u[k] = k == d ? v : 0.0;
                    sim3_exp(u, d == 6 ? (minus ? kSoExpM : kSoExpP) : 1.0, ex);
                    sim3_mul(ex, est, pe);
                }
                sim3_inverse(pe, pi);
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    s_est[tid][i] = pe[i];
                    s_inv[tid][i] = pi[i];
                }
            }
            __syncthreads();
            // computeActiveErrors + activeRobustChi2 + buildSystem
            const bool tap_edges = taps && round == 0 && iter == 0;
            seq_sums(std::integral_constant<int, kSoTerms>{}, [&](int c, double* row) {
                double X1[3], X2[3], o[4], w[2];
                load_pair(c, X1, X2, o, w);
                so_edge_terms(s_est, X2, o[0], o[1], cam1, w[0], delta, row, tap_edges, tap_err + 4 * c, tap_J + 28 * c);
                so_edge_terms(s_inv, X1, o[2], o[3], cam2, w[1], delta, row + kSoTerms, tap_edges, tap_err + 4 * c + 2,
                              tap_J + 28 * c + 14);
            });
            double h[28], bv[7];
            double currentChi = s_sum[0];
#pragma unroll
            for (int k = 0; k < 28; k++) h[k] = s_sum[1 + k];
#pragma unroll
            for (int k = 0; k < 7; k++) bv[k] = s_sum[29 + k];
            __syncthreads();   // s_sum is written again by the trial pass
            const double iniChi = currentChi;
            if (iter == 0) {
                double mx = 0;
#pragma unroll
                for (int j = 0; j < 7; j++) mx = fmax(fabs(h[lt_idx(j, j)]), mx);
                lm_init(lm, mx);
            }
            Sim3OptIter* rec = tap_it + min(n_lm, kSoLm - 1);
            if (taps && tid == 0) {
#pragma unroll
                for (int i = 0; i < 8; i++) rec->est[i] = est[i];
                rec->chi2 = currentChi;
#pragma unroll
                for (int k = 0; k < 28; k++) rec->H[k] = h[k];
#pragma unroll
                for (int k = 0; k < 7; k++) rec->b[k] = bv[k];
            }
            double rho = 0;
            int qmax = 0;
            do {
                double m[28], xs[7], te[8];
#pragma unroll
                for (int k = 0; k < 28; k++) m[k] = h[k];
#pragma unroll
                for (int j = 0; j < 7; j++) m[lt_idx(j, j)] += lm.lambda;
                const bool ok2 = ldlt_solve<7>(m, bv, xs);
                if (ok2) {   // VertexSim3Expmap::oplusImpl: Sim3(update) * estimate
                    double ex[8];
                    sim3_exp(xs, exp(xs[6]), ex);
                    sim3_mul(ex, est, te);
                } else {
#pragma unroll
                    for (int i = 0; i < 7; i++) xs[i] = 0.0;
#pragma unroll
                    for (int i = 0; i < 8; i++) te[i] = est[i];
                    npd++;
                }
                if (taps && tid == 0 && qmax < kSoTrials) {
#pragma unroll
                    for (int i = 0; i < 7; i++) rec->dx[qmax][i] = xs[i];
                }
                // computeActiveErrors at the trial estimate
                if (tid == 0) {
                    double ti[8];
                    sim3_inverse(te, ti);
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        s_est[0][i] = te[i];
                        s_inv[0][i] = ti[i];
                    }
                }
                __syncthreads();
                seq_sums(std::integral_constant<int, 1>{}, [&](int c, double* row) {
                    double X1[3], X2[3], o[4], w[2], e0, e1, rho1;
                    load_pair(c, X1, X2, o, w);
                    sim3_edge_error(s_est[0], X2, o[0], o[1], cam1, e0, e1);
                    huber(e0 * (w[0] * e0) + e1 * (w[0] * e1), delta, row[0], rho1);
                    sim3_edge_error(s_inv[0], X1, o[2], o[3], cam2, e0, e1);
                    huber(e0 * (w[1] * e0) + e1 * (w[1] * e1), delta, row[kSoTerms], rho1);
                });
                double tempChi = s_sum[0];
                __syncthreads();
#pragma unroll
                for (int i = 0; i < 8; i++) errest[i] = te[i];
                const LmTrial trial = lm_trial(lm, currentChi, tempChi, ok2, lm_scale(xs, lm.lambda, bv));
                rho = trial.rho;
                if (trial.accept) {
#pragma unroll
                    for (int i = 0; i < 8; i++) est[i] = te[i];
                }
                qmax++;
            } while (lm_retry(rho, qmax));
            if (taps && tid == 0) {
                rec->lambda = lm.lambda;
                rec->trials = qmax;
            }
            iters++;
            n_lm++;
            trials += qmax;
            if (lm_stop(lm, qmax, rho, iniChi, currentChi)) break;
        }
        if (tid == 0) {
            hdr->iters[round] = iters;
            hdr->trials[round] = trials;
            hdr->npd[round] = npd;
        }
        // the check (:930-949, :965-980): chi2() of the stored errors, those of
        // the last trial's estimate; a NaN keeps the pair
        if (tid == 0) {
            double ti[8];
            sim3_inverse(errest, ti);
#pragma unroll
            for (int i = 0; i < 8; i++) {
                s_est[0][i] = errest[i];
                s_inv[0][i] = ti[i];
                hdr->check_est[round][i] = errest[i];
            }
            s_cnt[0] = 0;
            s_cnt[1] = 0;
        }
        __syncthreads();
        int bad = 0, good = 0;
#pragma unroll 1
        for (int c = tid; c < n; c += kT) {
            if (gflag[c] != 0) continue;
            double X1[3], X2[3], o[4], w[2], e0, e1;
            load_pair(c, X1, X2, o, w);
            sim3_edge_error(s_est[0], X2, o[0], o[1], cam1, e0, e1);
            const double c12 = e0 * (w[0] * e0) + e1 * (w[0] * e1);
            sim3_edge_error(s_inv[0], X1, o[2], o[3], cam2, e0, e1);
            const double c21 = e0 * (w[1] * e0) + e1 * (w[1] * e1);
            if (taps) {
                tap_chi[((long long)round * L.cap + c) * 2] = c12;
                tap_chi[((long long)round * L.cap + c) * 2 + 1] = c21;
            }
            if (c12 > th2 || c21 > th2) {
                gflag[c] = (uint8_t)(round + 1);
                bad++;
            } else {
                good++;
            }
        }
        if (bad) atomicAdd(&s_cnt[0], bad);
        if (good) atomicAdd(&s_cnt[1], good);
        __syncthreads();
        const int nb = s_cnt[0], ng = s_cnt[1];
        __syncthreads();
        if (round == 0) {
            n_bad = nb;
            if (n - n_bad < 10) {   // return 0 at once: g2oS12 is not updated (:957-958)
                early = 1;
                break;
            }
        } else {
            n_in = ng;
        }
    }
    if (n == 0) early = 1;
    if (tid == 0) {
        double R[9];
        qmat(Q{est[0], est[1], est[2], est[3]}, R);   // Eigen's toRotationMatrix
#pragma unroll
        for (int i = 0; i < 8; i++) hdr->est[i] = est[i];
#pragma unroll
        for (int i = 0; i < 9; i++) hdr->R12[i] = (float)R[i];
#pragma unroll
        for (int i = 0; i < 3; i++) hdr->t12[i] = (float)est[4 + i];
        hdr->s12 = (float)est[7];
        hdr->n_in = early ? 0 : n_in;
        hdr->n_bad = n_bad;
        hdr->early = early;
        hdr->n_lm = n_lm;
    }
}

}  // namespace orbx

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
using namespace orbx;

namespace {

bool finite_all(const float* v, int n)
{
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// What every form checks of a query's own fields.
int check_common(const orbx_sim3_opt_query& q)
{
    if (!q.matches12 && q.n1 > 0) return ORBX_ERR_ARG;
    if (!(q.th2 > 0.f) || !std::isfinite(q.th2)) return ORBX_ERR_ARG;
    if (!finite_all(q.R12, 9) || !finite_all(q.t12, 3) || !std::isfinite(q.s12)) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// The correspondences of :844-923 in i order: matches12[i] >= 0, both map
// points good.  ORBX_ERR_ARG for a match index >= n2.
int correspondences(const int32_t* m, int n1, int n2, const uint8_t* v1, int good1, const uint8_t* v2, int good2,
                    std::vector<int32_t>* ci, std::vector<int32_t>* cj)
{
    for (int i = 0; i < n1; i++) {
        const int i2 = m[i];
        if (i2 >= n2) return ORBX_ERR_ARG;   // the reference would read past KF2's keypoints
        if (i2 < 0) continue;
        const bool ok1 = good1 ? v1[i] == good1 : v1[i] != 0;
        const bool ok2 = good2 ? v2[i2] == good2 : v2[i2] != 0;
        if (ok1 && ok2) {
            ci->push_back(i);
            cj->push_back(i2);
        }
    }
    return ORBX_OK;
}

bool any_corr_tap(const orbx_sim3_opt_query& q)
{
    return q.corr_index || q.x3dc1 || q.x3dc2 || q.edge_err || q.edge_J || q.edge_chi2;
}

bool any_tap(const orbx_sim3_opt_query& q)
{
    return any_corr_tap(q) || q.it_est || q.it_chi2 || q.it_H || q.it_b || q.it_lambda || q.it_trials || q.it_dx ||
           q.check_est;
}

// One candidate's block (host copy) into the query's outputs and taps.
void scatter(const uint8_t* blk, const Sim3OptLayout& L, const std::vector<int32_t>& ci, bool taps,
             orbx_sim3_opt_query* q)
{
    const Sim3OptHdr* h = reinterpret_cast<const Sim3OptHdr*>(blk);
    const int n = (int)ci.size();
    q->n_corr = n;
    q->n_bad = h->n_bad;
    q->n_in = h->n_in;
    q->returned_early = h->early;
    q->n_lm = h->n_lm;
    for (int r = 0; r < 2; r++) {
        q->iterations[r] = h->iters[r];
        q->trials[r] = h->trials[r];
        q->not_posdef[r] = h->npd[r];
    }
    const uint8_t* flag = blk + L.o_flag;
    for (int c = 0; c < n; c++)
        if (flag[c]) q->matches12[ci[c]] = -1;
    if (!h->early) {
        std::memcpy(q->q12, h->est, 4 * sizeof(double));
        std::memcpy(q->t12d, h->est + 4, 3 * sizeof(double));
        q->s12d = h->est[7];
        std::memcpy(q->R12, h->R12, sizeof(q->R12));
        std::memcpy(q->t12, h->t12, sizeof(q->t12));
        q->s12 = h->s12;
    }
    if (q->corr_index && n) std::memcpy(q->corr_index, ci.data(), (size_t)n * 4);
    if (q->x3dc1 && n) std::memcpy(q->x3dc1, blk + L.o_x1, (size_t)n * 12);
    if (q->x3dc2 && n) std::memcpy(q->x3dc2, blk + L.o_x2, (size_t)n * 12);
    if (!taps) return;
    if (q->edge_err && n) std::memcpy(q->edge_err, blk + L.o_err, (size_t)n * 32);
    if (q->edge_J && n) std::memcpy(q->edge_J, blk + L.o_J, (size_t)n * 224);
    if (q->edge_chi2) {
        const double* chi = reinterpret_cast<const double*>(blk + L.o_chi);
        const int rounds = h->early ? 1 : 2;
        for (int r = 0; r < rounds && n > 0; r++)
            for (int c = 0; c < n; c++)
                if (flag[c] == 0 || flag[c] > r)   // tested in round r
                    std::memcpy(q->edge_chi2 + ((size_t)r * q->cap + c) * 2, chi + ((size_t)r * L.cap + c) * 2, 16);
    }
    const Sim3OptIter* it = reinterpret_cast<const Sim3OptIter*>(blk + L.o_it);
    for (int k = 0; k < std::min<int>(h->n_lm, kSoLm); k++) {
        if (q->it_est) std::memcpy(q->it_est + 8 * k, it[k].est, 64);
        if (q->it_chi2) q->it_chi2[k] = it[k].chi2;
        if (q->it_H) std::memcpy(q->it_H + 28 * k, it[k].H, 224);
        if (q->it_b) std::memcpy(q->it_b + 7 * k, it[k].b, 56);
        if (q->it_lambda) q->it_lambda[k] = it[k].lambda;
        if (q->it_trials) q->it_trials[k] = it[k].trials;
        if (q->it_dx) {   // the trials that ran; zeros behind them
            double* dx = q->it_dx + (size_t)kSoTrials * 7 * k;
            const int t = std::max(0, std::min<int>(it[k].trials, kSoTrials));
            std::memset(dx, 0, sizeof(it[k].dx));
            std::memcpy(dx, it[k].dx, (size_t)t * 7 * sizeof(double));
        }
    }
    if (q->check_est && n > 0) std::memcpy(q->check_est, h->check_est, (h->early ? 1 : 2) * 64);
}

// The out fields of a candidate without correspondences: no kernel work.
void scatter_empty(orbx_sim3_opt_query* q)
{
    q->n_corr = q->n_bad = q->n_in = q->n_lm = 0;
    q->returned_early = 1;
    for (int r = 0; r < 2; r++) q->iterations[r] = q->trials[r] = q->not_posdef[r] = 0;
}

void fill_prob(Sim3OptProb& d, const orbx_sim3_opt_query& q, int n, int nlevels, const float* T1w, const float* T2w,
               const float* cam1, const float* cam2, bool taps)
{
    d.n = n;
    d.nlevels = nlevels;
    d.taps = taps ? 1 : 0;
    d.pad = 0;
    std::memcpy(d.T1w, T1w, 48);
    std::memcpy(d.T2w, T2w, 48);
    std::memcpy(d.cam1, cam1, 16);
    std::memcpy(d.cam2, cam2, 16);
    std::memcpy(d.R12, q.R12, 36);
    std::memcpy(d.t12, q.t12, 12);
    d.s12 = q.s12;
    d.th2 = q.th2;
    d.delta = (double)std::sqrt(q.th2);   // const float deltaHuber = sqrt(th2) (:840)
}

// Where one candidate's arrays lie in the call's packed inputs.
struct Sim3OptStaged {
    Region<orbx_keypoint> k1, k2;   // host form only: the slot form reads the context's keypoints
    Region<int32_t> ci, cj;
    Region<float> pos1, pos2, isig1, sig2;   // taken in this order
};

void point_prob(Sim3OptProb& d, const PackedStage& st, const Sim3OptStaged& a)
{
    d.ci = st.dev(a.ci);
    d.cj = st.dev(a.cj);
    d.pos1 = st.dev(a.pos1);
    d.pos2 = st.dev(a.pos2);
    d.isig1 = st.dev(a.isig1);
    d.sig2 = st.dev(a.sig2);
}

// Upload, launch (a lone candidate gets the wide workgroup), read back and scatter.
int run_sim3opt(PackedStage& st, Region<Sim3OptProb> descs, const Sim3OptLayout& L,
                const std::vector<std::vector<int32_t>>& ci, bool taps, orbx_sim3_opt_query* qs)
{
    orbx_ctx* ctx = st.ctx;
    const int P = (int)descs.count;
    int r = st.upload();
    if (r != ORBX_OK) return r;
    ResultBlocks res(ctx, st.behind(), P, L.stride);
    timer_begin(ctx, "sim3opt");
    if (P == 1)
        hipLaunchKernelGGL(k_sim3_opt<kSoWide>, dim3(1), dim3(64 * kSoWide), 0, ctx->stream, st.dev(descs), res.dev, L);
    else
        hipLaunchKernelGGL(k_sim3_opt<1>, dim3(P), dim3(64), 0, ctx->stream, st.dev(descs), res.dev, L);
    timer_end(ctx, "sim3opt");
    ORBX_HIP_CHECK(hipGetLastError());
    if ((r = res.read()) != ORBX_OK) return r;
    for (int k = 0; k < P; k++) {
        if (ci[k].empty()) scatter_empty(&qs[k]);
        else scatter(res.block(k), L, ci[k], taps, &qs[k]);
    }
    return ORBX_OK;
}

}  // namespace

extern "C" int orbx_optimize_sim3_batch(orbx_ctx* ctx, int B, orbx_sim3_opt_query* qs)
{
    if (!ctx || !qs || B < 1) return ORBX_ERR_ARG;
    // argument rules, before any device work; what travels is taken as it is checked:
    // descriptors | per candidate: keypoints, correspondence lists, positions, level tables
    std::vector<std::vector<int32_t>> ci(B), cj(B);
    std::vector<Sim3OptStaged> at(B);
    int cap = 1, work = 0;
    bool taps = false;
    PackedStage st(ctx);
    const Region<Sim3OptProb> descs = st.take<Sim3OptProb>(B);
    for (int b = 0; b < B; b++) {
        const orbx_sim3_opt_query& q = qs[b];
        if (q.n1 < 0 || q.n2 < 0 || (q.n1 > 0 && (!q.keys1 || !q.pos1 || !q.valid1)) ||
            (q.n2 > 0 && (!q.keys2 || !q.pos2 || !q.valid2)) || !q.T1w || !q.T2w || !q.cam1 || !q.cam2 ||
            !q.inv_sigma2_1 || !q.sigma2_2)
            return ORBX_ERR_ARG;
        int r = check_common(q);
        if (r != ORBX_OK) return r;
        if (q.nlevels < 1 || q.nlevels > kMaxLevels) return ORBX_ERR_ARG;
        if (q.n1 > kMaxFeatures || q.n2 > kMaxFeatures) return ORBX_ERR_UNSUPPORTED;
        if (!octaves_ok(q.keys1, q.n1, q.nlevels) || !octaves_ok(q.keys2, q.n2, q.nlevels)) return ORBX_ERR_ARG;
        if ((r = correspondences(q.matches12, q.n1, q.n2, q.valid1, 0, q.valid2, 0, &ci[b], &cj[b])) != ORBX_OK) return r;
        const int n = (int)ci[b].size();
        if (any_corr_tap(q) && q.cap < n) return ORBX_ERR_CAPACITY;
        taps = taps || any_tap(q);
        cap = std::max(cap, n);
        work += n > 0;
        at[b] = {st.take(q.n1, q.keys1), st.take(q.n2, q.keys2), st.take(n, ci[b].data()), st.take(n, cj[b].data()),
                 st.take((size_t)q.n1 * 3, q.pos1), st.take((size_t)q.n2 * 3, q.pos2),
                 st.take(q.nlevels, q.inv_sigma2_1), st.take(q.nlevels, q.sigma2_2)};
    }
    if (work == 0) {
        for (int b = 0; b < B; b++) scatter_empty(&qs[b]);
        return ORBX_OK;
    }
    ctx_enter(ctx);
    const Sim3OptLayout L = sim3opt_layout(cap, taps);
    int r = st.open((size_t)B * L.stride);
    if (r != ORBX_OK) return r;
    for (int b = 0; b < B; b++) {
        const orbx_sim3_opt_query& q = qs[b];
        Sim3OptProb& d = st.host(descs)[b];
        d.k1 = st.dev(at[b].k1);
        d.k2 = st.dev(at[b].k2);
        point_prob(d, st, at[b]);
        fill_prob(d, q, (int)ci[b].size(), q.nlevels, q.T1w, q.T2w, q.cam1, q.cam2, taps);
    }
    return run_sim3opt(st, descs, L, ci, taps, qs);
}

extern "C" int orbx_optimize_sim3(orbx_ctx* ctx, orbx_sim3_opt_query* q) { return orbx_optimize_sim3_batch(ctx, 1, q); }

extern "C" int orbx_dev_optimize_sim3(orbx_ctx* ctx, int slot1, const orbx_sim3_kf* kf1, const float* inv_sigma2_1, int n,
                                      const int* slots2, const orbx_sim3_kf* kf2s, orbx_sim3_opt_query* out)
{
    if (!ctx || n < 0) return ORBX_ERR_ARG;
    if (n == 0) return ORBX_OK;
    auto kf_ok = [&](const orbx_sim3_kf* k) {
        return k && k->mp && k->pos && k->Tcw && k->cam && k->nlevels == ctx->geom.nlevels && k->nlevels >= 1 &&
               k->nlevels <= kMaxLevels;
    };
    auto slot_ok = [&](int s) { return s >= 0 && s < ctx->slots; };
    if (!kf_ok(kf1) || !inv_sigma2_1 || !slots2 || !kf2s || !out || !slot_ok(slot1)) return ORBX_ERR_ARG;
    for (int k = 0; k < n; k++) {
        if (!kf_ok(&kf2s[k]) || !kf2s[k].sigma2 || !slot_ok(slots2[k]) || !out[k].matches12) return ORBX_ERR_ARG;
        const int r = check_common(out[k]);
        if (r != ORBX_OK) return r;
    }
    const int nf = ctx->geom.nfeatures;
    if (nf > kMaxFeatures) return ORBX_ERR_UNSUPPORTED;
    ctx_enter(ctx);
    // the slots' feature counts bound the arrays the caller passes
    std::vector<int32_t> cnt;
    int r = read_slot_counts(ctx, cnt);
    if (r != ORBX_OK) return r;
    auto count = [&](int slot) { return std::max(0, std::min<int>(cnt[slot], nf)); };
    const int n1 = count(slot1);
    const int nl = kf1->nlevels;
    std::vector<std::vector<int32_t>> ci(n), cj(n);
    std::vector<Sim3OptStaged> at(n);
    int cap = 1, work = 0;
    bool taps = false;
    // what travels: descriptors | KF1: positions, inverse sigma2 | per candidate: lists, positions, sigma2
    PackedStage st(ctx);
    const Region<Sim3OptProb> descs = st.take<Sim3OptProb>(n);
    const Region<float> pos1 = st.take((size_t)n1 * 3, kf1->pos), isig1 = st.take(nl, inv_sigma2_1);
    for (int k = 0; k < n; k++) {
        const int n2 = count(slots2[k]);
        if ((r = correspondences(out[k].matches12, n1, n2, kf1->mp, 1, kf2s[k].mp, 1, &ci[k], &cj[k])) != ORBX_OK) return r;
        const int nc = (int)ci[k].size();
        if (any_corr_tap(out[k]) && out[k].cap < nc) return ORBX_ERR_CAPACITY;
        taps = taps || any_tap(out[k]);
        cap = std::max(cap, nc);
        work += nc > 0;
        at[k] = {{}, {}, st.take(nc, ci[k].data()), st.take(nc, cj[k].data()), pos1,
                 st.take((size_t)n2 * 3, kf2s[k].pos), isig1, st.take(nl, kf2s[k].sigma2)};
    }
    if (work == 0) {
        for (int k = 0; k < n; k++) scatter_empty(&out[k]);
        return ORBX_OK;
    }
    const Sim3OptLayout L = sim3opt_layout(cap, taps);
    if ((r = st.open((size_t)n * L.stride)) != ORBX_OK) return r;
    for (int k = 0; k < n; k++) {
        Sim3OptProb& d = st.host(descs)[k];
        d.k1 = slot_frame_dev(ctx, slot1, nullptr).kps;
        d.k2 = slot_frame_dev(ctx, slots2[k], nullptr).kps;
        point_prob(d, st, at[k]);
        fill_prob(d, out[k], (int)ci[k].size(), nl, kf1->Tcw, kf2s[k].Tcw, kf1->cam, kf2s[k].cam, taps);
    }
    return run_sim3opt(st, descs, L, ci, taps, out);
}
