// The g2o pieces the FP64 optimisers share (orbx_pose.hip, orbx_sim3opt.hip,
// orbx_lba.hip, orbx_essgraph.hip): the Huber kernel, Eigen's pivoted LDLT behind
// LinearSolverDense, and OptimizationAlgorithmLevenberg's control with
// ORB-SLAM's stop rule.  Every kernel has to follow the oracle's trajectory
// bit for bit, so this is the one text of each expression: operand order,
// pow(x, 3) and the fmin / fmax argument order are g2o's and stay as they are
// (the build has -ffp-contract=off, so the same text gives the same bits in
// every kernel).  All of it is inline arithmetic on scalars; forced inline,
// so no kernel's code depends on the inliner's view of its surroundings.
// The oracle (oracle/ref_pose.cpp, ref_lba.cpp) and the tests' numpy
// restatements keep texts of their own on purpose: they are what this one is
// checked against.
#pragma once

#include <hip/hip_runtime.h>

namespace orbx {

#define ORBX_LM_FN __device__ __forceinline__

constexpr double kDblMax = 1.79769313486231570815e+308;   // std::numeric_limits<double>::max()
constexpr double kDblMin = 2.2250738585072014e-308;       // std::numeric_limits<double>::min()

// Pinhole intrinsics of an edge's camera, widened to double.
struct CamD {
    double fx, fy, cx, cy;
};

// Packed lower triangle: entry (i, j), j <= i, at i (i + 1) / 2 + j.
constexpr int lt_idx(int i, int j) { return i * (i + 1) / 2 + j; }

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91)
ORBX_LM_FN void huber(double e2, double delta, double& rho0, double& rho1)
{
    const double dsqr = delta * delta;
    if (e2 <= dsqr) {
        rho0 = e2;
        rho1 = 1.;
    } else {
        const double sq = sqrt(e2);
        rho0 = 2 * sq * delta - dsqr;
        rho1 = delta / sq;
    }
}

// Eigen::LDLT<MatrixXd> of the lower triangle of m (packed, N x N) and the
// solve of m x = b: the restatement of oracle/ref_pose.cpp ldlt_solve with
// every index a compile-time constant (the runtime pivot selects among
// unrolled swap variants), so the matrix stays in registers.  False when the
// matrix is indefinite (LinearSolverDense's isPositive test).
template <int N>
ORBX_LM_FN bool ldlt_solve(double (&m)[N * (N + 1) / 2], const double (&b)[N], double (&x)[N])
{
    int tr[N];
    double temp[N];
    int sign = 0;   // 0 zero, 1 positive semidefinite, 2 negative semidefinite, 3 indefinite
    auto swap_d = [](double& a, double& c) {
        const double t = a;
        a = c;
        c = t;
    };
#pragma unroll
    for (int k = 0; k < N; k++) {
        int big = k;
        double bv = fabs(m[lt_idx(k, k)]);
#pragma unroll
        for (int i = k + 1; i < N; i++)
            if (fabs(m[lt_idx(i, i)]) > bv) {
                bv = fabs(m[lt_idx(i, i)]);
                big = i;
            }
        tr[k] = big;
#pragma unroll
        for (int q = k + 1; q < N; q++) {
            if (big == q) {
#pragma unroll
                for (int j = 0; j < k; j++) swap_d(m[lt_idx(k, j)], m[lt_idx(q, j)]);
#pragma unroll
                for (int i = q + 1; i < N; i++) swap_d(m[lt_idx(i, k)], m[lt_idx(i, q)]);
                swap_d(m[lt_idx(k, k)], m[lt_idx(q, q)]);
#pragma unroll
                for (int i = k + 1; i < q; i++) swap_d(m[lt_idx(i, k)], m[lt_idx(q, i)]);
            }
        }
        if (k > 0) {
#pragma unroll
            for (int j = 0; j < k; j++) temp[j] = m[lt_idx(j, j)] * m[lt_idx(k, j)];
            double acc = m[lt_idx(k, 0)] * temp[0];
#pragma unroll
            for (int j = 1; j < k; j++) acc += m[lt_idx(k, j)] * temp[j];
            m[lt_idx(k, k)] -= acc;
#pragma unroll
            for (int i = k + 1; i < N; i++)
#pragma unroll
                for (int j = 0; j < k; j++) m[lt_idx(i, k)] -= m[lt_idx(i, j)] * temp[j];
        }
        const double akk = m[lt_idx(k, k)];
        if (k < N - 1 && fabs(akk) > 0.0) {
#pragma unroll
            for (int i = k + 1; i < N; i++) m[lt_idx(i, k)] /= akk;
        }
        if (sign == 1) {
            if (akk < 0) sign = 3;
        } else if (sign == 2) {
            if (akk > 0) sign = 3;
        } else if (sign == 0) {
            if (akk > 0) sign = 1;
            else if (akk < 0) sign = 2;
        }
    }
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = b[i];
#pragma unroll
    for (int k = 0; k < N; k++)
#pragma unroll
        for (int q = k + 1; q < N; q++)
            if (tr[k] == q) swap_d(x[k], x[q]);
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < i; j++) x[i] -= m[lt_idx(i, j)] * x[j];
#pragma unroll
    for (int i = 0; i < N; i++) {
        if (fabs(m[lt_idx(i, i)]) > kDblMin) x[i] /= m[lt_idx(i, i)];
        else x[i] = 0.0;
    }
#pragma unroll
    for (int i = N - 2; i >= 0; i--) {
        double s = m[lt_idx(i + 1, i)] * x[i + 1];
#pragma unroll
        for (int j = i + 2; j < N; j++) s += m[lt_idx(j, i)] * x[j];
        x[i] -= s;
    }
#pragma unroll
    for (int k = N - 1; k >= 0; k--)
#pragma unroll
        for (int q = k + 1; q < N; q++)
            if (tr[k] == q) swap_d(x[k], x[q]);
    return sign == 1 || sign == 0;
}

// ---------------------------------------------------------------------------
// OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp
// :61-164) as the reference runs it: the damping state, the decision on one
// trial and the end of an iteration.  What a kernel does with the decision
// (adopt the trial estimate or system, pop the saved poses and points)
// differs per kernel and stays at the call site.
// ---------------------------------------------------------------------------
struct LmState {
    double lambda, ni;   // _currentLambda, _ni
    int nBad;            // ORB-SLAM's nBad (levenberg.cpp:154-161)
};

constexpr int kLmMaxTrials = 10;   // _maxTrialsAfterFailure

// computeLambdaInit (levenberg.cpp:166-180) from the largest |diagonal entry|
// of the Hessian, at the first iteration of an optimize() call.
ORBX_LM_FN void lm_init(LmState& s, double max_diag)
{
    s.lambda = 1e-5 * max_diag;   // _tau
    s.ni = 2;
    s.nBad = 0;
}

// computeLambdaInit with setUserLambdaInit(lambda) (levenberg.cpp:166-169): the
// caller's value instead of _tau times the largest diagonal entry.
ORBX_LM_FN void lm_init_user(LmState& s, double lambda)
{
    s.lambda = lambda;
    s.ni = 2;
    s.nBad = 0;
}

// computeScale's sum (levenberg.cpp:182-189) over a dense N-vector step; the
// local-BA kernels form theirs as a block sum and hand lm_trial the total.
template <int N>
ORBX_LM_FN double lm_scale(const double (&x)[N], double lambda, const double (&b)[N])
{
    double scale = 0;
#pragma unroll
    for (int j = 0; j < N; j++) scale += x[j] * (lambda * x[j] + b[j]);
    return scale;
}

struct LmTrial {
    bool accept;
    double rho;
};

// One trial's outcome (levenberg.cpp:126-147).  tempChi: the robust chi2 at the
// trial state; ok: the linear solve succeeded; scale: computeScale's sum.
// An accepted trial's chi2 becomes currentChi and the damping relaxes; a
// rejected one multiplies it by ni.
ORBX_LM_FN LmTrial lm_trial(LmState& s, double& currentChi, double tempChi, bool ok, double scale)
{
    if (!ok) tempChi = kDblMax;
    scale += 1e-3;   // :131, after computeScale
    const double rho = (currentChi - tempChi) / scale;
    const bool accept = rho > 0 && isfinite(tempChi);
    // on copies, stored once below: a store through a reference inside a
    // branch keeps the branch, and the kernels' code has selects here
    double lambda = s.lambda, ni = s.ni, chi = currentChi;
    if (accept) {
        double alpha = 1. - pow((2 * rho - 1), 3);
        alpha = fmin(alpha, 2. / 3.);   // _goodStepUpperScale
        lambda *= fmax(1. / 3., alpha);   // _goodStepLowerScale
        ni = 2;
        chi = tempChi;
    } else {
        lambda *= ni;
        ni *= 2;
    }
    s.lambda = lambda;
    s.ni = ni;
    currentChi = chi;
    return {accept, rho};
}

// The trial loop's condition (levenberg.cpp:149); the local-BA kernels add
// the caller's abort flag (_optimizer->terminate()).
ORBX_LM_FN bool lm_retry(double rho, int qmax) { return rho < 0 && qmax < kLmMaxTrials; }

// The end of an iteration: true when the optimisation stops.  g2o's
// Terminated (no trial accepted, or rho == 0) and ORB-SLAM's rule
// (levenberg.cpp:151-161): three iterations running that gain less than
// 1e-3 of their initial chi2.
ORBX_LM_FN bool lm_stop(LmState& s, int qmax, double rho, double iniChi, double currentChi)
{
    if (qmax == kLmMaxTrials || rho == 0) return true;
    int nBad = s.nBad;   // a copy, stored once (see lm_trial)
    if ((iniChi - currentChi) * 1e3 < iniChi) nBad++;
    else nBad = 0;
    s.nBad = nBad;
    return nBad >= 3;
}

#undef ORBX_LM_FN

}  // namespace orbx
