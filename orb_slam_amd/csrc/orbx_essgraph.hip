// Optimizer::OptimizeEssentialGraph on MI355X (FP64): the 7-DoF pose graph of
// LoopClosing::CorrectLoop (src/Optimizer.cc:540-789) over every keyframe of
// the map, the Sim3 -> SE3 recovery of the poses and the correction of the
// map points.
//
// g2o subset (as the reference configures it): one VertexSim3Expmap per
// keyframe, the loop keyframe fixed; EdgeSim3 with information I7 and error
// (C * v0 * v1.inverse()).log(); no robust kernel; BaseBinaryEdge's central
// differences with delta = 1e-9 on both vertices (base_binary_edge.hpp
// :131-205); BlockSolver_7_3 with no marginalised vertex, so no Schur step: a
// sparse Cholesky of H + lambda I; OptimizationAlgorithmLevenberg with
// setUserLambdaInit(1e-16), optimize(20) and ORB-SLAM's stop rule.
//
// Mapping.  The arithmetic is in the linearisation, about 29 Sim3 logarithms
// per edge and iteration, and that is edge-parallel over the whole device:
//   k_eg_perturb    a thread per (keyframe, k): the 15 estimates of one
//                   linearisation (the current one and Sim3(+-delta e_d) * S)
//                   and their inverses;
//   k_eg_linearize  a thread per edge: the error, the 28 perturbed errors, Ji,
//                   Jj and the edge's 120 terms (the lower triangles of Ji^T Ji
//                   and Jj^T Jj, Ji^T Jj, -Ji^T e, -Jj^T e, e^T e);
//   k_eg_assemble   a workgroup per block row, a lane per entry of a 7 x 7
//                   block: the diagonal block and b as sequential sums over
//                   the vertex's incidence list (g2o's edge order, built on
//                   the host), each off-diagonal block the sum over the edges
//                   joining the pair;
//   k_eg_begin      one workgroup: chi2 as the sequential sum over the edges,
//                   lambda at the first iteration, the per-iteration taps.
// A trial is
//   k_eg_solve      one workgroup through global memory: H + lambda I into the
//                   factor's copy (H survives: g2o's restoreDiagonal), the
//                   block Cholesky over the envelope column by column -- the
//                   diagonal 7 x 7, then every row of the column in parallel,
//                   a thread per (row, line of the block) -- and the forward
//                   and back substitutions; a pivot that is not positive and
//                   finite fails the solve (a zero step, the trial rejected);
//   k_eg_update     a thread per keyframe: Sim3(dx) * estimate and its inverse;
//   k_eg_error      a thread per edge: e^T e at the trial estimates;
//   k_eg_decide     one workgroup: the trial's chi2 and computeScale as
//                   sequential sums, then one thread takes the Levenberg
//                   decision (orbx_lm.h) and the workgroup adopts the trial
//                   estimates on acceptance.
// The host reads the small state after each trial and queues the next trial,
// the next iteration or the end.  No floating-point atomics and no grid-wide
// barrier anywhere: every sum has an order fixed by the problem (edge order,
// ascending block column, ascending row), so two runs give the same bytes
// whatever the launch shapes, the taps or the timer do.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "orbx_device.h"
#include "orbx_essgraph_host.h"
#include "orbx_internal.h"
#include "orbx_lm.h"
#include "orbx_se3.h"
#include "orbx_sim3_dev.h"
#include "orbx_stage.h"

namespace orbx {

constexpr int kEgLm = ORBX_ESSGRAPH_MAX_LM;
constexpr int kEgTerms = 120;   // per edge: 28 + 28 of the diagonal blocks, 49 of Ji^T Jj, 7 + 7 of b, chi2
constexpr int kEgOffJj = 28, kEgOffM = 56, kEgOffB = 105, kEgOffChi = 119;
constexpr int kEgWg = 256;      // threads of the one-workgroup kernels
constexpr double kEgLambdaInit = 1e-16;   // setUserLambdaInit (src/Optimizer.cc:553)

struct EgState {
    double lambda, ni, currentChi, iniChi, rho, chi2_first;
    int32_t nBad, qmax, iters, trials, npd, ok, retry, stop;
};

struct EgDev {
    const orbx_essgraph_kf* kfs;
    const orbx_essgraph_edge* edges;
    const float* pos;
    const int32_t* ref;
    const int32_t *free_of_kf, *kf_of_free, *first, *col_rows, *inc_off, *inc_edge;
    const int64_t *row_off, *col_off;
    int n_kf, n_edges, n_points, n_free, fixed, taps;
    long long n_blocks;
    double *vscw, *swc, *est, *trial, *trial_inv, *pert, *pert_inv, *meas, *terms, *chi_e, *H, *L, *b, *y, *dx;
    EgState* state;
    float *Tcw_out, *pos_out;
    double *edge_err, *edge_J, *it_chi2, *it_lambda, *it_est, *it_b, *it_dx, *it_Hdiag;
    int32_t* it_trials;
};

// vScw of a keyframe (:578-590): CorrectedSim3 where the map has one, else
// Sim3(toMatrix3d(R), toVector3d(t), 1.0) -- widened floats, Eigen's
// quaternion of the matrix, never renormalised.
__device__ inline void eg_scw(const orbx_essgraph_kf& k, double o[8])
{
    if (k.has_corrected) {
#pragma unroll
        for (int i = 0; i < 8; i++) o[i] = k.corrected[i];
        return;
    }
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (double)k.Tcw[i];
    const Q q = qfrom(R);
    o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
#pragma unroll
    for (int i = 0; i < 3; i++) o[4 + i] = (double)k.Tcw[9 + i];
    o[7] = 1.0;
}

// EdgeSim3::computeError (types_seven_dof_expmap.h:106-114)
__device__ inline int eg_edge_error(const double* C, const double* vi, const double* vj_inv, double e[7])
{
    double a[8], b[8];
    sim3_mul(C, vi, a);
    sim3_mul(a, vj_inv, b);
    return sim3_log(b, e);
}

// vScw and the first estimate per keyframe, the measurement per edge (:609-729).
__global__ __launch_bounds__(64) void k_eg_setup(EgDev D)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < D.n_kf) {
        double s[8];
        eg_scw(D.kfs[t], s);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            D.vscw[8 * (long long)t + i] = s[i];
            D.est[8 * (long long)t + i] = s[i];
        }
    }
    if (t < D.n_edges) {
        const orbx_essgraph_edge E = D.edges[t];
        const orbx_essgraph_kf& ki = D.kfs[E.i];
        const orbx_essgraph_kf& kj = D.kfs[E.j];
        double si[8], sj[8], swi[8], m[8];
        if (E.kind == 1 && ki.has_noncorrected) {
#pragma unroll
            for (int i = 0; i < 8; i++) si[i] = ki.noncorrected[i];
        } else {
            eg_scw(ki, si);
        }
        if (E.kind == 1 && kj.has_noncorrected) {
#pragma unroll
            for (int i = 0; i < 8; i++) sj[i] = kj.noncorrected[i];
        } else {
            eg_scw(kj, sj);
        }
        sim3_inverse(si, swi);
        sim3_mul(sj, swi, m);   // Sji = Sjw * Swi
#pragma unroll
        for (int i = 0; i < 8; i++) D.meas[8 * (long long)t + i] = m[i];
    }
}

// The 15 estimates of one linearisation per keyframe and their inverses; a
// keyframe outside the system has the current one only.
__global__ __launch_bounds__(64) void k_eg_perturb(EgDev D)
{
    const long long g = (long long)blockIdx.x * 64 + threadIdx.x;
    if (g >= (long long)D.n_kf * 15) return;
    const int v = (int)(g / 15), k = (int)(g % 15);
    if (k > 0 && D.free_of_kf[v] < 0) return;
    double est[8], pe[8], pi[8];
#pragma unroll
    for (int i = 0; i < 8; i++) est[i] = D.est[8 * (long long)v + i];
    if (k == 0) {
#pragma unroll
        for (int i = 0; i < 8; i++) pe[i] = est[i];
    } else {
        const int d = (k - 1) >> 1;
        const bool minus = ((k - 1) & 1) != 0;
        const double dv = minus ? -kSoDelta : kSoDelta;
        double u[7], ex[8];
#pragma unroll
        for (int i = 0; i < 7; i++) u[i] = i == d ? dv : 0.0;
        sim3_exp(u, d == 6 ? (minus ? kSoExpM : kSoExpP) : 1.0, ex);
        sim3_mul(ex, est, pe);
    }
    sim3_inverse(pe, pi);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        D.pert[g * 8 + i] = pe[i];
        D.pert_inv[g * 8 + i] = pi[i];
    }
}

// computeError and linearizeOplus of one edge, then constructQuadraticForm's
// products with Omega = I (base_binary_edge.hpp:91-113).  A fixed side has a
// zero Jacobian and contributes zero terms, which nothing reads.
__global__ __launch_bounds__(64) void k_eg_linearize(EgDev D, int tap)
{
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= D.n_edges) return;
    constexpr double scalar = 1.0 / (2 * kSoDelta);
    const orbx_essgraph_edge E = D.edges[e];
    const bool fi = D.free_of_kf[E.i] >= 0, fj = D.free_of_kf[E.j] >= 0;
    const double* Pi = D.pert + (long long)E.i * 15 * 8;
    const double* PIj = D.pert_inv + (long long)E.j * 15 * 8;
    double C[8], err[7], Ji[49], Jj[49];
#pragma unroll
    for (int i = 0; i < 8; i++) C[i] = D.meas[8 * (long long)e + i];
    eg_edge_error(C, Pi, PIj, err);
#pragma unroll
    for (int i = 0; i < 49; i++) Ji[i] = Jj[i] = 0.0;
#pragma unroll 1
    for (int side = 0; side < 2; side++) {
        if (!(side == 0 ? fi : fj)) continue;
#pragma unroll 1
        for (int d = 0; d < 7; d++) {
            double ep[7], em[7];
            if (side == 0) {
                eg_edge_error(C, Pi + (1 + 2 * d) * 8, PIj, ep);
                eg_edge_error(C, Pi + (2 + 2 * d) * 8, PIj, em);
            } else {
                eg_edge_error(C, Pi, PIj + (1 + 2 * d) * 8, ep);
                eg_edge_error(C, Pi, PIj + (2 + 2 * d) * 8, em);
            }
            double* J = side == 0 ? Ji : Jj;
#pragma unroll
            for (int k = 0; k < 7; k++) J[k * 7 + d] = scalar * (ep[k] - em[k]);
        }
    }
    if (tap) {
#pragma unroll
        for (int k = 0; k < 7; k++) D.edge_err[7 * (long long)e + k] = err[k];
        for (int k = 0; k < 49; k++) {
            D.edge_J[98 * (long long)e + k] = Ji[k];
            D.edge_J[98 * (long long)e + 49 + k] = Jj[k];
        }
    }
    double* T = D.terms + (long long)e * kEgTerms;
    for (int a = 0; a < 7; a++)
        for (int b = 0; b <= a; b++) {
            double hi = Ji[a] * Ji[b], hj = Jj[a] * Jj[b];
            for (int k = 1; k < 7; k++) {
                hi += Ji[k * 7 + a] * Ji[k * 7 + b];
                hj += Jj[k * 7 + a] * Jj[k * 7 + b];
            }
            T[lt_idx(a, b)] = hi;
            T[kEgOffJj + lt_idx(a, b)] = hj;
        }
    for (int p = 0; p < 7; p++)
        for (int q = 0; q < 7; q++) {
            double m = Ji[p] * Jj[q];
            for (int k = 1; k < 7; k++) m += Ji[k * 7 + p] * Jj[k * 7 + q];
            T[kEgOffM + p * 7 + q] = m;
        }
    for (int a = 0; a < 7; a++) {   // b += J^T omega_r, omega_r = -(Omega e)
        double bi = Ji[a] * -err[0], bj = Jj[a] * -err[0];
        for (int k = 1; k < 7; k++) {
            bi += Ji[k * 7 + a] * -err[k];
            bj += Jj[k * 7 + a] * -err[k];
        }
        T[kEgOffB + a] = bi;
        T[kEgOffB + 7 + a] = bj;
    }
    double chi = err[0] * err[0];
#pragma unroll
    for (int k = 1; k < 7; k++) chi += err[k] * err[k];
    T[kEgOffChi] = chi;
}

// One block row of H and b.  Lane t < 49 owns entry (t / 7, t % 7) of every
// block of the row; only this workgroup writes the row.
__global__ __launch_bounds__(64) void k_eg_assemble(EgDev D)
{
    const int r = blockIdx.x, tid = threadIdx.x;
    if (r >= D.n_free) return;
    const int fr = D.first[r];
    double* row = D.H + D.row_off[r] * 49;
    for (int k = tid; k < (r - fr + 1) * 49; k += 64) row[k] = 0.0;
    __syncthreads();
    if (tid >= 49) return;
    const int p = tid / 7, q = tid % 7;
    const int dl = p >= q ? lt_idx(p, q) : lt_idx(q, p);
    double diag = 0.0, bacc = 0.0;
    for (int k = D.inc_off[r]; k < D.inc_off[r + 1]; k++) {
        const int e = D.inc_edge[k] >> 1, side = D.inc_edge[k] & 1;
        const double* T = D.terms + (long long)e * kEgTerms;
        diag += T[side * kEgOffJj + dl];
        if (tid < 7) bacc += T[kEgOffB + side * 7 + tid];
        const orbx_essgraph_edge E = D.edges[e];
        const int c = D.free_of_kf[side ? E.i : E.j];
        if (c >= fr && c < r) {   // H_ij = Ji^T Jj; the lower block of the pair is its transpose when j's row holds it
            double* blk = row + (long long)(c - fr) * 49;
            blk[tid] += side == 0 ? T[kEgOffM + p * 7 + q] : T[kEgOffM + q * 7 + p];
        }
    }
    row[(long long)(r - fr) * 49 + tid] = diag;
    if (tid < 7) D.b[7 * (long long)r + tid] = bacc;
}

// The strictly sequential sum of term(0..n) from +0.0: the workgroup stages
// kEgWg terms in LDS, thread 0 adds them in order.  Valid in thread 0.
template <typename F>
__device__ inline double eg_seq_sum(long long n, double* s_buf, F&& term)
{
    double acc = 0.0;
    for (long long g = 0; g < n; g += kEgWg) {
        const long long k = g + threadIdx.x;
        s_buf[threadIdx.x] = k < n ? term(k) : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = (int)min((long long)kEgWg, n - g);
            for (int j = 0; j < cnt; j++) acc += s_buf[j];
        }
        __syncthreads();
    }
    return acc;
}

// The start of an iteration (levenberg.cpp:75-92): currentChi, lambda at the
// first one, the taps.
__global__ __launch_bounds__(kEgWg) void k_eg_begin(EgDev D)
{
    __shared__ double s_buf[kEgWg];
    const int tid = threadIdx.x;
    const double* terms = D.terms;
    const double chi = eg_seq_sum(D.n_edges, s_buf, [&](long long e) { return terms[e * kEgTerms + kEgOffChi]; });
    EgState* S = D.state;
    const int it = min(S->iters, kEgLm - 1);
    if (tid == 0) {
        S->currentChi = chi;
        S->iniChi = chi;
        if (S->iters == 0) {
            LmState lm;
            lm_init_user(lm, kEgLambdaInit);
            S->lambda = lm.lambda;
            S->ni = lm.ni;
            S->nBad = lm.nBad;
            S->chi2_first = chi;
        }
        S->rho = 0;
        S->qmax = 0;
        if (D.taps) D.it_chi2[it] = chi;
    }
    if (!D.taps) return;
    for (long long k = tid; k < (long long)D.n_kf * 8; k += kEgWg) D.it_est[(long long)it * D.n_kf * 8 + k] = D.est[k];
    for (long long k = tid; k < (long long)D.n_free * 7; k += kEgWg) D.it_b[(long long)it * D.n_free * 7 + k] = D.b[k];
    for (long long k = tid; k < (long long)D.n_free * 28; k += kEgWg) {
        const int r = (int)(k / 28), l = (int)(k % 28);
        int p = 0;
        while (lt_idx(p + 1, 0) <= l) p++;
        const int q = l - lt_idx(p, 0);
        D.it_Hdiag[(long long)it * D.n_free * 28 + k] = D.H[(D.row_off[r + 1] - 1) * 49 + p * 7 + q];
    }
}

// (H + lambda I) dx = b over the envelope: the factor L L^T into the copy,
// L y = b, L^T dx = y.  Every block is 7 x 7 row-major; row r's block of
// column k lies at (row_off[r] + k - first[r]) * 49.  Sums run over ascending
// block column, then ascending inner index, one subtraction at a time.
__global__ __launch_bounds__(kEgWg) void k_eg_solve(EgDev D)
{
    __shared__ double s_d[49], s_v[7];
    __shared__ int s_fail;
    const int tid = threadIdx.x, n = D.n_free;
    double* L = D.L;
    double* y = D.y;
    EgState* S = D.state;
    const double lambda = S->lambda;
    for (long long k = tid; k < D.n_blocks * 49; k += kEgWg) L[k] = D.H[k];
    for (long long k = tid; k < (long long)n * 7; k += kEgWg) y[k] = D.b[k];
    if (tid == 0) s_fail = 0;
    __syncthreads();
    for (long long k = tid; k < (long long)n * 7; k += kEgWg) L[(D.row_off[k / 7 + 1] - 1) * 49 + (k % 7) * 8] += lambda;
    __syncthreads();
    for (int c = 0; c < n; c++) {
        const int fc = D.first[c];
        double* Lc = L + D.row_off[c] * 49;
        if (tid < 49) {   // the diagonal block less the row's own products
            const int p = tid / 7, q = tid % 7;
            double acc = Lc[(long long)(c - fc) * 49 + tid];
            if (q <= p)
                for (int k = fc; k < c; k++) {
                    const double* blk = Lc + (long long)(k - fc) * 49;
                    for (int m = 0; m < 7; m++) acc -= blk[p * 7 + m] * blk[q * 7 + m];
                }
            s_d[tid] = acc;
        }
        __syncthreads();
        if (tid == 0) {   // its 7 x 7 Cholesky, in registers: every index below is a constant
            double l[49];
#pragma unroll
            for (int i = 0; i < 49; i++) l[i] = s_d[i];
            bool bad = false;
#pragma unroll
            for (int j = 0; j < 7; j++) {
                double v = l[j * 7 + j];
#pragma unroll
                for (int m = 0; m < j; m++) v -= l[j * 7 + m] * l[j * 7 + m];
                bad = bad || !(v > 0.0) || !isfinite(v);   // what follows a bad pivot is not used
                const double d = sqrt(v);
                l[j * 7 + j] = d;
#pragma unroll
                for (int i = j + 1; i < 7; i++) {
                    double w = l[i * 7 + j];
#pragma unroll
                    for (int m = 0; m < j; m++) w -= l[i * 7 + m] * l[j * 7 + m];
                    l[i * 7 + j] = w / d;
                }
            }
#pragma unroll
            for (int i = 0; i < 7; i++)
#pragma unroll
                for (int j = 0; j < 7; j++) s_d[i * 7 + j] = j <= i ? l[i * 7 + j] : 0.0;
            if (bad) s_fail = 1;
        }
        __syncthreads();
        if (s_fail) break;
        if (tid < 49) Lc[(long long)(c - fc) * 49 + tid] = s_d[tid];
        // every row of the column: L(r, c) = (A(r, c) - sum_k L(r, k) L(c, k)^T) L(c, c)^-T
        const long long c0 = D.col_off[c];
        const int cnt = (int)(D.col_off[c + 1] - c0);
        for (int w = tid; w < cnt * 7; w += kEgWg) {
            const int r = D.col_rows[c0 + w / 7], p = w % 7;
            const int fr = D.first[r];
            double* Lr = L + D.row_off[r] * 49;
            double* dst = Lr + (long long)(c - fr) * 49 + p * 7;
            double s[7];
            for (int q = 0; q < 7; q++) s[q] = dst[q];
            for (int k = max(fr, fc); k < c; k++) {
                const double* a = Lr + (long long)(k - fr) * 49 + p * 7;
                const double* bk = Lc + (long long)(k - fc) * 49;
                for (int q = 0; q < 7; q++)
                    for (int m = 0; m < 7; m++) s[q] -= a[m] * bk[q * 7 + m];
            }
            for (int q = 0; q < 7; q++) {
                double v = s[q];
                for (int m = 0; m < q; m++) v -= s[m] * s_d[q * 7 + m];
                s[q] = v / s_d[q * 7 + q];
            }
            for (int q = 0; q < 7; q++) dst[q] = s[q];
        }
        __syncthreads();
    }
    const bool ok = s_fail == 0;
    if (ok) {
        for (int c = 0; c < n; c++) {   // L y = b, column by column
            const double* dg = L + (D.row_off[c + 1] - 1) * 49;
            if (tid == 0) {   // the block and the right-hand side into registers first: one wait, then the chain
                double l[49], v[7];
#pragma unroll
                for (int i = 0; i < 49; i++) l[i] = dg[i];
#pragma unroll
                for (int p = 0; p < 7; p++) v[p] = y[7 * (long long)c + p];
#pragma unroll
                for (int p = 0; p < 7; p++) {
#pragma unroll
                    for (int m = 0; m < p; m++) v[p] -= l[p * 7 + m] * v[m];
                    v[p] = v[p] / l[p * 7 + p];
                }
#pragma unroll
                for (int p = 0; p < 7; p++) {
                    s_v[p] = v[p];
                    y[7 * (long long)c + p] = v[p];
                }
            }
            __syncthreads();
            const long long c0 = D.col_off[c];
            const int cnt = (int)(D.col_off[c + 1] - c0);
            for (int w = tid; w < cnt * 7; w += kEgWg) {
                const int r = D.col_rows[c0 + w / 7], p = w % 7;
                const double* a = L + (D.row_off[r] + c - D.first[r]) * 49 + p * 7;
                double v = y[7 * (long long)r + p];
                for (int m = 0; m < 7; m++) v -= a[m] * s_v[m];
                y[7 * (long long)r + p] = v;
            }
            __syncthreads();
        }
        for (int r = n - 1; r >= 0; r--) {   // L^T dx = y, row by row from the last
            const int fr = D.first[r];
            const double* Lr = L + D.row_off[r] * 49;
            const double* dg = Lr + (long long)(r - fr) * 49;
            if (tid == 0) {
                double l[49], v[7];
#pragma unroll
                for (int i = 0; i < 49; i++) l[i] = dg[i];
#pragma unroll
                for (int q = 0; q < 7; q++) v[q] = y[7 * (long long)r + q];
#pragma unroll
                for (int q = 6; q >= 0; q--) {
#pragma unroll
                    for (int m = q + 1; m < 7; m++) v[q] -= l[m * 7 + q] * v[m];
                    v[q] = v[q] / l[q * 7 + q];
                }
#pragma unroll
                for (int q = 0; q < 7; q++) {
                    s_v[q] = v[q];
                    y[7 * (long long)r + q] = v[q];
                }
            }
            __syncthreads();
            for (int w = tid; w < (r - fr) * 7; w += kEgWg) {
                const int k = fr + w / 7, q = w % 7;
                const double* blk = Lr + (long long)(k - fr) * 49;
                double v = y[7 * (long long)k + q];
                for (int p = 0; p < 7; p++) v -= blk[p * 7 + q] * s_v[p];
                y[7 * (long long)k + q] = v;
            }
            __syncthreads();
        }
    }
    for (long long k = tid; k < (long long)n * 7; k += kEgWg) D.dx[k] = ok ? y[k] : 0.0;
    if (tid == 0) {
        S->ok = ok ? 1 : 0;
        if (!ok) S->npd++;
    }
}

// VertexSim3Expmap::oplusImpl per keyframe of the system: Sim3(dx) * estimate.
__global__ __launch_bounds__(64) void k_eg_update(EgDev D)
{
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= D.n_kf) return;
    double est[8], te[8], ti[8];
#pragma unroll
    for (int i = 0; i < 8; i++) est[i] = D.est[8 * (long long)v + i];
    const int f = D.free_of_kf[v];
    if (f >= 0) {
        double u[7], ex[8];
#pragma unroll
        for (int i = 0; i < 7; i++) u[i] = D.dx[7 * (long long)f + i];
        sim3_exp(u, exp(u[6]), ex);
        sim3_mul(ex, est, te);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) te[i] = est[i];
    }
    sim3_inverse(te, ti);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        D.trial[8 * (long long)v + i] = te[i];
        D.trial_inv[8 * (long long)v + i] = ti[i];
    }
}

// computeActiveErrors at the trial estimates: chi2 per edge.
__global__ __launch_bounds__(64) void k_eg_error(EgDev D)
{
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= D.n_edges) return;
    const orbx_essgraph_edge E = D.edges[e];
    double err[7];
    eg_edge_error(D.meas + 8 * (long long)e, D.trial + 8 * (long long)E.i, D.trial_inv + 8 * (long long)E.j, err);
    double chi = err[0] * err[0];
#pragma unroll
    for (int k = 1; k < 7; k++) chi += err[k] * err[k];
    D.chi_e[e] = chi;
}

// One trial's outcome (levenberg.cpp:126-161) and the end of an iteration.
__global__ __launch_bounds__(kEgWg) void k_eg_decide(EgDev D)
{
    __shared__ double s_buf[kEgWg];
    __shared__ int s_accept, s_it;
    const int tid = threadIdx.x;
    EgState* S = D.state;
    const double lambda = S->lambda;
    const double* chi_e = D.chi_e;
    const double* dx = D.dx;
    const double* b = D.b;
    const double tempChi = eg_seq_sum(D.n_edges, s_buf, [&](long long e) { return chi_e[e]; });
    const double scale =
        eg_seq_sum((long long)D.n_free * 7, s_buf, [&](long long j) { return dx[j] * (lambda * dx[j] + b[j]); });
    if (tid == 0) {
        const int it = s_it = min(S->iters, kEgLm - 1);   // before the iteration is counted
        LmState lm{S->lambda, S->ni, S->nBad};
        double currentChi = S->currentChi;
        const LmTrial trial = lm_trial(lm, currentChi, tempChi, S->ok != 0, scale);
        const int qmax = S->qmax + 1;
        const bool retry = lm_retry(trial.rho, qmax);
        bool stop = false;
        if (!retry) {
            stop = lm_stop(lm, qmax, trial.rho, S->iniChi, currentChi);
            S->iters++;
            S->trials += qmax;
            if (D.taps) {
                D.it_lambda[it] = lm.lambda;
                D.it_trials[it] = qmax;
            }
        }
        S->lambda = lm.lambda;
        S->ni = lm.ni;
        S->nBad = lm.nBad;
        S->currentChi = currentChi;
        S->rho = trial.rho;
        S->qmax = qmax;
        S->retry = retry ? 1 : 0;
        S->stop = stop ? 1 : 0;
        s_accept = trial.accept ? 1 : 0;
    }
    __syncthreads();
    if (s_accept)
        for (long long k = tid; k < (long long)D.n_kf * 8; k += kEgWg) D.est[k] = D.trial[k];
    if (D.taps)
        for (long long k = tid; k < (long long)D.n_free * 7; k += kEgWg) D.it_dx[(long long)s_it * D.n_free * 7 + k] = dx[k];
}

// SE3 pose recovery (:737-755): [sR t; 0 1] -> [R t/s; 0 1], and vCorrectedSwc.
__global__ __launch_bounds__(64) void k_eg_recover(EgDev D)
{
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= D.n_kf) return;
    double est[8], inv[8], R[9];
#pragma unroll
    for (int i = 0; i < 8; i++) est[i] = D.est[8 * (long long)v + i];
    sim3_inverse(est, inv);
    qmat(Q{est[0], est[1], est[2], est[3]}, R);
    const double f = 1. / est[7];
    float* out = D.Tcw_out + 12 * (long long)v;
#pragma unroll
    for (int i = 0; i < 9; i++) out[i] = (float)R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) out[9 + i] = (float)(est[4 + i] * f);
#pragma unroll
    for (int i = 0; i < 8; i++) D.swc[8 * (long long)v + i] = inv[i];
}

// Point correction (:758-788): correctedSwr.map(Srw.map(P)).
__global__ __launch_bounds__(64) void k_eg_points(EgDev D)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= D.n_points) return;
    const int r = D.ref[k];
    if (r < 0 || r >= D.n_kf) return;
    const double P[3] = {(double)D.pos[3 * (long long)k], (double)D.pos[3 * (long long)k + 1],
                         (double)D.pos[3 * (long long)k + 2]};
    double c[3], w[3];
    sim3_map(D.vscw + 8 * (long long)r, P, c);
    sim3_map(D.swc + 8 * (long long)r, c, w);
#pragma unroll
    for (int i = 0; i < 3; i++) D.pos_out[3 * (long long)k + i] = (float)w[i];
}

}  // namespace orbx

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
using namespace orbx;

namespace {

bool eg_sim3_ok(const double* s)
{
    for (int i = 0; i < 8; i++)
        if (!std::isfinite(s[i])) return false;
    return s[7] > 0;
}

int eg_check_query(const orbx_essgraph_query& q, std::vector<int64_t>* ids)
{
    if (q.n_kf < 1 || q.n_edges < 0 || q.n_points < 0 || !q.kfs || !q.Tcw_out) return ORBX_ERR_ARG;
    if (q.n_edges > 0 && !q.edges) return ORBX_ERR_ARG;
    if (q.n_points > 0 && (!q.pos || !q.ref_kf || !q.pos_out)) return ORBX_ERR_ARG;
    if (q.loop_kf < 0 || q.loop_kf >= q.n_kf || q.cur_kf < 0 || q.cur_kf >= q.n_kf) return ORBX_ERR_ARG;
    if (q.n_kf > ORBX_ESSGRAPH_MAX_KF) return ORBX_ERR_UNSUPPORTED;
    ids->resize(q.n_kf);
    for (int k = 0; k < q.n_kf; k++) {
        const orbx_essgraph_kf& kf = q.kfs[k];
        (*ids)[k] = kf.id;
        for (int i = 0; i < 12; i++)
            if (!std::isfinite(kf.Tcw[i])) return ORBX_ERR_ARG;
        if (kf.has_corrected && !eg_sim3_ok(kf.corrected)) return ORBX_ERR_ARG;
        if (kf.has_noncorrected && !eg_sim3_ok(kf.noncorrected)) return ORBX_ERR_ARG;
    }
    const int r = essgraph_check(q.n_kf, ids->data(), q.loop_kf, q.n_edges, q.edges);
    if (r != ORBX_OK) return r;
    for (int k = 0; k < q.n_points; k++) {
        if (q.ref_kf[k] < -1 || q.ref_kf[k] >= q.n_kf) return ORBX_ERR_ARG;
        if (q.ref_kf[k] >= 0)
            for (int i = 0; i < 3; i++)
                if (!std::isfinite(q.pos[3 * (size_t)k + i])) return ORBX_ERR_ARG;
    }
    return ORBX_OK;
}

bool eg_any_tap(const orbx_essgraph_query& q)
{
    return q.edge_meas || q.edge_err || q.edge_J || q.it_chi2 || q.it_lambda || q.it_trials || q.it_est || q.it_b ||
           q.it_dx || q.it_Hdiag;
}

template <typename T>
T* eg_at(uint8_t* base, long long off)
{
    return reinterpret_cast<T*>(base + off);
}

inline unsigned eg_groups(long long n) { return (unsigned)std::max<long long>(1, (n + 63) / 64); }

}  // namespace

extern "C" int orbx_essgraph_plan(int n_kf, const int64_t* ids, int fixed, int n_edges, const orbx_essgraph_edge* edges,
                                  int32_t* free_index, int32_t* first, int64_t* row_off, int* n_free,
                                  long long* n_blocks, int* max_row_blocks)
{
    const int r = essgraph_check(n_kf, ids, fixed, n_edges, edges);
    if (r != ORBX_OK) return r;
    const EssPlan P = essgraph_plan(n_kf, ids, fixed, n_edges, edges);
    if (free_index) std::copy(P.free_of_kf.begin(), P.free_of_kf.end(), free_index);
    if (first) std::copy(P.first.begin(), P.first.end(), first);
    if (row_off) std::copy(P.row_off.begin(), P.row_off.end(), row_off);
    if (n_free) *n_free = P.n_free;
    if (n_blocks) *n_blocks = P.n_blocks;
    if (max_row_blocks) *max_row_blocks = P.max_row_blocks;
    return ORBX_OK;
}

extern "C" int orbx_optimize_essential_graph(orbx_ctx* ctx, orbx_essgraph_query* q)
{
    if (!ctx || !q) return ORBX_ERR_ARG;
    std::vector<int64_t> ids;
    int r = eg_check_query(*q, &ids);
    if (r != ORBX_OK) return r;
    if (essgraph_blocks(q->n_kf, ids.data(), q->loop_kf, q->n_edges, q->edges) * 49 * 8 > ORBX_ESSGRAPH_MAX_FACTOR_BYTES)
        return ORBX_ERR_UNSUPPORTED;
    const EssPlan P = essgraph_plan(q->n_kf, ids.data(), q->loop_kf, q->n_edges, q->edges);
    const bool taps = eg_any_tap(*q);
    const int nk = q->n_kf, ne = q->n_edges, np = q->n_points, nf = P.n_free;

    // what travels: keyframes, edges, points | the plan
    PackedStage st(ctx);
    const auto kfs = st.take(nk, q->kfs);
    const auto edges = st.take(ne, q->edges);
    const auto pos = st.take((size_t)np * 3, q->pos);
    const auto ref = st.take(np, q->ref_kf);
    const auto free_of_kf = st.take(nk, P.free_of_kf.data());
    const auto kf_of_free = st.take(nf, P.kf_of_free.data());
    const auto first = st.take(nf, P.first.data());
    const auto col_rows = st.take(P.col_rows.size(), P.col_rows.data());
    const auto inc_off = st.take(nf + 1, P.inc_off.data());
    const auto inc_edge = st.take(P.inc_edge.size(), P.inc_edge.data());
    const auto row_off = st.take(nf + 1, P.row_off.data());
    const auto col_off = st.take(nf + 1, P.col_off.data());
    // behind them: the read-back range (state, estimates, poses, points, taps), then device-only scratch
    BlockOffsets o;
    const long long o_state = o.take(sizeof(EgState));
    const long long o_est = o.take((long long)nk * 64);
    const long long o_tcw = o.take((long long)nk * 48);
    const long long o_pout = o.take((long long)np * 12);
    const long long o_meas = o.take((long long)ne * 64);
    const long long o_eerr = o.take(taps ? (long long)ne * 56 : 0);
    const long long o_eJ = o.take(taps ? (long long)ne * 98 * 8 : 0);
    const long long o_ichi = o.take(taps ? kEgLm * 8 : 0);
    const long long o_ilam = o.take(taps ? kEgLm * 8 : 0);
    const long long o_itr = o.take(taps ? kEgLm * 4 : 0);
    const long long o_iest = o.take(taps ? (long long)kEgLm * nk * 64 : 0);
    const long long o_ib = o.take(taps ? (long long)kEgLm * nf * 56 : 0);
    const long long o_idx = o.take(taps ? (long long)kEgLm * nf * 56 : 0);
    const long long o_ihd = o.take(taps ? (long long)kEgLm * nf * 28 * 8 : 0);
    const long long readback = taps ? o.end : o_meas;
    const long long o_vscw = o.take((long long)nk * 64);
    const long long o_swc = o.take((long long)nk * 64);
    const long long o_trial = o.take((long long)nk * 64);
    const long long o_tinv = o.take((long long)nk * 64);
    const long long o_pert = o.take((long long)nk * 15 * 64);
    const long long o_pinv = o.take((long long)nk * 15 * 64);
    const long long o_terms = o.take((long long)ne * kEgTerms * 8);
    const long long o_chi = o.take((long long)ne * 8);
    const long long o_H = o.take(P.n_blocks * 49 * 8);
    const long long o_L = o.take(P.n_blocks * 49 * 8);
    const long long o_b = o.take((long long)nf * 56);
    const long long o_y = o.take((long long)nf * 56);
    const long long o_dx = o.take((long long)nf * 56);

    ctx_enter(ctx);
    st.align_end(16);
    if ((r = st.open((size_t)o.end)) != ORBX_OK) return r;
    if ((r = ensure_pinned(ctx, sizeof(EgState))) != ORBX_OK) return r;
    if ((r = st.upload()) != ORBX_OK) return r;
    uint8_t* B = st.behind();
    EgDev D{};
    D.kfs = st.dev(kfs);
    D.edges = st.dev(edges);
    D.pos = st.dev(pos);
    D.ref = st.dev(ref);
    D.free_of_kf = st.dev(free_of_kf);
    D.kf_of_free = st.dev(kf_of_free);
    D.first = st.dev(first);
    D.col_rows = st.dev(col_rows);
    D.inc_off = st.dev(inc_off);
    D.inc_edge = st.dev(inc_edge);
    D.row_off = st.dev(row_off);
    D.col_off = st.dev(col_off);
    D.n_kf = nk;
    D.n_edges = ne;
    D.n_points = np;
    D.n_free = nf;
    D.fixed = q->loop_kf;
    D.taps = taps ? 1 : 0;
    D.n_blocks = P.n_blocks;
    D.state = eg_at<EgState>(B, o_state);
    D.est = eg_at<double>(B, o_est);
    D.Tcw_out = eg_at<float>(B, o_tcw);
    D.pos_out = eg_at<float>(B, o_pout);
    D.meas = eg_at<double>(B, o_meas);
    D.edge_err = eg_at<double>(B, o_eerr);
    D.edge_J = eg_at<double>(B, o_eJ);
    D.it_chi2 = eg_at<double>(B, o_ichi);
    D.it_lambda = eg_at<double>(B, o_ilam);
    D.it_trials = eg_at<int32_t>(B, o_itr);
    D.it_est = eg_at<double>(B, o_iest);
    D.it_b = eg_at<double>(B, o_ib);
    D.it_dx = eg_at<double>(B, o_idx);
    D.it_Hdiag = eg_at<double>(B, o_ihd);
    D.vscw = eg_at<double>(B, o_vscw);
    D.swc = eg_at<double>(B, o_swc);
    D.trial = eg_at<double>(B, o_trial);
    D.trial_inv = eg_at<double>(B, o_tinv);
    D.pert = eg_at<double>(B, o_pert);
    D.pert_inv = eg_at<double>(B, o_pinv);
    D.terms = eg_at<double>(B, o_terms);
    D.chi_e = eg_at<double>(B, o_chi);
    D.H = eg_at<double>(B, o_H);
    D.L = eg_at<double>(B, o_L);
    D.b = eg_at<double>(B, o_b);
    D.y = eg_at<double>(B, o_y);
    D.dx = eg_at<double>(B, o_dx);

    hipStream_t s = ctx->stream;
    EgState host{};
    timer_begin(ctx, "essgraph");
    ORBX_HIP_CHECK(hipMemsetAsync(B, 0, (size_t)readback, s));   // the state, and defined bytes wherever nothing is written
    hipLaunchKernelGGL(k_eg_setup, dim3(eg_groups(std::max(nk, ne))), dim3(64), 0, s, D);
    for (int it = 0; it < kEgLm && nf > 0; it++) {
        timer_begin(ctx, "essgraph.linearize");
        hipLaunchKernelGGL(k_eg_perturb, dim3(eg_groups((long long)nk * 15)), dim3(64), 0, s, D);
        hipLaunchKernelGGL(k_eg_linearize, dim3(eg_groups(ne)), dim3(64), 0, s, D, taps && it == 0 ? 1 : 0);
        hipLaunchKernelGGL(k_eg_assemble, dim3(nf), dim3(64), 0, s, D);
        hipLaunchKernelGGL(k_eg_begin, dim3(1), dim3(kEgWg), 0, s, D);
        timer_end(ctx, "essgraph.linearize");
        do {
            timer_begin(ctx, "essgraph.factor");
            hipLaunchKernelGGL(k_eg_solve, dim3(1), dim3(kEgWg), 0, s, D);
            timer_end(ctx, "essgraph.factor");
            hipLaunchKernelGGL(k_eg_update, dim3(eg_groups(nk)), dim3(64), 0, s, D);
            hipLaunchKernelGGL(k_eg_error, dim3(eg_groups(ne)), dim3(64), 0, s, D);
            hipLaunchKernelGGL(k_eg_decide, dim3(1), dim3(kEgWg), 0, s, D);
            ORBX_HIP_CHECK(hipGetLastError());
            ORBX_HIP_CHECK(hipMemcpyAsync(ctx->host_pinned, D.state, sizeof(EgState), hipMemcpyDeviceToHost, s));
            ORBX_HIP_CHECK(hipStreamSynchronize(s));
            std::memcpy(&host, ctx->host_pinned, sizeof(EgState));
        } while (host.retry && host.qmax < kLmMaxTrials);
        if (host.stop) break;
    }
    timer_begin(ctx, "essgraph.points");
    hipLaunchKernelGGL(k_eg_recover, dim3(eg_groups(nk)), dim3(64), 0, s, D);
    if (np > 0) hipLaunchKernelGGL(k_eg_points, dim3(eg_groups(np)), dim3(64), 0, s, D);
    timer_end(ctx, "essgraph.points");
    timer_end(ctx, "essgraph");
    ORBX_HIP_CHECK(hipGetLastError());
    std::vector<uint8_t> back((size_t)readback);
    ORBX_HIP_CHECK(hipMemcpyAsync(back.data(), B, (size_t)readback, hipMemcpyDeviceToHost, s));
    ORBX_HIP_CHECK(hipStreamSynchronize(s));

    uint8_t* h = back.data();
    std::memcpy(&host, h + o_state, sizeof(EgState));
    q->iterations = host.iters;
    q->trials = host.trials;
    q->not_posdef = host.npd;
    q->chi2_first = host.chi2_first;
    q->chi2_last = host.currentChi;
    q->lambda_last = host.lambda;
    q->n_free = nf;
    q->n_blocks = P.n_blocks;
    q->max_row_blocks = P.max_row_blocks;
    std::memcpy(q->Tcw_out, h + o_tcw, (size_t)nk * 48);
    if (q->est_out) std::memcpy(q->est_out, h + o_est, (size_t)nk * 64);
    for (int k = 0; k < np; k++)
        if (q->ref_kf[k] >= 0) std::memcpy(q->pos_out + 3 * (size_t)k, h + o_pout + 12 * (size_t)k, 12);
    if (!taps) return ORBX_OK;
    const size_t its = (size_t)std::min<int>(host.iters, kEgLm);
    if (q->edge_meas && ne) std::memcpy(q->edge_meas, h + o_meas, (size_t)ne * 64);
    if (q->edge_err && ne && its) std::memcpy(q->edge_err, h + o_eerr, (size_t)ne * 56);
    if (q->edge_J && ne && its) std::memcpy(q->edge_J, h + o_eJ, (size_t)ne * 98 * 8);
    if (q->it_chi2) std::memcpy(q->it_chi2, h + o_ichi, its * 8);
    if (q->it_lambda) std::memcpy(q->it_lambda, h + o_ilam, its * 8);
    if (q->it_trials) std::memcpy(q->it_trials, h + o_itr, its * 4);
    if (q->it_est) std::memcpy(q->it_est, h + o_iest, its * nk * 64);
    if (q->it_b) std::memcpy(q->it_b, h + o_ib, its * nf * 56);
    if (q->it_dx) std::memcpy(q->it_dx, h + o_idx, its * nf * 56);
    if (q->it_Hdiag) std::memcpy(q->it_Hdiag, h + o_ihd, its * nf * 28 * 8);
    return ORBX_OK;
}
