// g2o::Sim3 on the device (Thirdparty/g2o/g2o/types/sim3/sim3.h), FP64, shared
// by the Sim3 optimisation (orbx_sim3opt.hip) and the essential-graph
// optimisation (orbx_essgraph.hip): the exponential, the product, the inverse,
// the logarithm, and the constants of BaseBinaryEdge's central differences.
#pragma once

#include <hip/hip_runtime.h>

#include "orbx_se3.h"

namespace orbx {

constexpr double kSoDelta = 1e-9;   // base_binary_edge.hpp:133
constexpr double kSoExpP = 0x1.000000044b830p+0;   // exp(+1e-9), correctly rounded
constexpr double kSoExpM = 0x1.fffffff768fa1p-1;   // exp(-1e-9)

// g2o::Sim3 as (x, y, z, w, tx, ty, tz, s).
// Sim3(const Vector7d& update) (sim3.h:70-142); es = exp(update[6]).
__device__ inline void sim3_exp(const double u[7], double es, double out[8])
{
    const double om[3] = {u[0], u[1], u[2]}, up[3] = {u[3], u[4], u[5]};
    const double sigma = u[6];
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    double O2[9], R[9], W[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) O2[i * 3 + j] = O[i * 3] * O[j] + O[i * 3 + 1] * O[3 + j] + O[i * 3 + 2] * O[6 + j];
    const double s = es;
    const double eps = 0.00001;
    double A, B, C;
    bool rodrigues;
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.;
            B = 1. / 6.;
            rodrigues = false;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
            rodrigues = true;
        }
    } else {
        C = (s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
            rodrigues = false;
        } else {
            const double a = s * sin(theta);
            const double b = s * cos(theta);
            const double theta2 = theta * theta;
            const double sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
            rodrigues = true;
        }
    }
    if (rodrigues) {
        const double ra = sin(theta) / theta, rb = (1 - cos(theta)) / (theta * theta);
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + ra * O[i] + rb * O2[i];
    } else {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + O[i] + O2[i];
    }
    const Q q = qfrom(R);
#pragma unroll
    for (int i = 0; i < 9; i++) W[i] = A * O[i] + B * O2[i] + C * (i % 4 == 0 ? 1.0 : 0.0);
    out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
#pragma unroll
    for (int i = 0; i < 3; i++) out[4 + i] = W[i * 3] * up[0] + W[i * 3 + 1] * up[1] + W[i * 3 + 2] * up[2];
    out[7] = s;
}

// Sim3::operator* (sim3.h:266-272): the quaternion is never renormalised
__device__ inline void sim3_mul(const double a[8], const double b[8], double o[8])
{
    const Q qa{a[0], a[1], a[2], a[3]};
    const Q r = qmul(qa, Q{b[0], b[1], b[2], b[3]});
    const double bt[3] = {b[4], b[5], b[6]};
    double rt[3];
    qrot(qa, bt, rt);
    o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
#pragma unroll
    for (int i = 0; i < 3; i++) o[4 + i] = a[7] * rt[i] + a[4 + i];
    o[7] = a[7] * b[7];
}

// Sim3::inverse (sim3.h:233-236)
__device__ inline void sim3_inverse(const double a[8], double o[8])
{
    const Q rc{-a[0], -a[1], -a[2], a[3]};
    const double f = -1. / a[7];
    const double st[3] = {f * a[4], f * a[5], f * a[6]};
    double rt[3];
    qrot(rc, st, rt);
    o[0] = rc.x; o[1] = rc.y; o[2] = rc.z; o[3] = rc.w;
    o[4] = rt[0]; o[5] = rt[1]; o[6] = rt[2];
    o[7] = 1. / a[7];
}

// Sim3::map (sim3.h:144-146)
__device__ inline void sim3_map(const double a[8], const double p[3], double o[3])
{
    double r[3];
    qrot(Q{a[0], a[1], a[2], a[3]}, p, r);
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = a[7] * r[i] + a[4 + i];
}

// W.lu().solve(t) of a 3 x 3 (row-major m, overwritten): Eigen's PartialPivLU
// in its unblocked order -- per column the pivot search by |.| down the column
// (the first largest wins), the row swap, the column scaled by the pivot, the
// rank-1 update -- then the permuted right-hand side through the unit-lower
// forward and the upper back substitution, each row's dot product summed
// before it is subtracted.  The swaps are spelled out per case, so every index
// is a constant.
__device__ inline void lu3_solve(double m[9], const double b[3], double x[3])
{
    double c0 = b[0], c1 = b[1], c2 = b[2];
    auto swap_d = [](double& p, double& q) {
        const double t = p;
        p = q;
        q = t;
    };
    {
        int p = 0;
        double big = fabs(m[0]);
        if (fabs(m[3]) > big) {
            big = fabs(m[3]);
            p = 1;
        }
        if (fabs(m[6]) > big) {
            big = fabs(m[6]);
            p = 2;
        }
        if (p == 1) {
            swap_d(m[0], m[3]); swap_d(m[1], m[4]); swap_d(m[2], m[5]); swap_d(c0, c1);
        } else if (p == 2) {
            swap_d(m[0], m[6]); swap_d(m[1], m[7]); swap_d(m[2], m[8]); swap_d(c0, c2);
        }
        if (big != 0.0) {
            m[3] /= m[0];
            m[6] /= m[0];
        }
        m[4] -= m[3] * m[1]; m[5] -= m[3] * m[2];
        m[7] -= m[6] * m[1]; m[8] -= m[6] * m[2];
    }
    {
        const double big = fmax(fabs(m[4]), fabs(m[7]));
        if (fabs(m[7]) > fabs(m[4])) {
            swap_d(m[3], m[6]); swap_d(m[4], m[7]); swap_d(m[5], m[8]); swap_d(c1, c2);
        }
        if (big != 0.0) m[7] /= m[4];
        m[8] -= m[7] * m[5];
    }
    c1 -= m[3] * c0;
    c2 -= m[6] * c0 + m[7] * c1;
    x[2] = c2 / m[8];
    x[1] = (c1 - m[5] * x[2]) / m[4];
    x[0] = (c0 - (m[1] * x[1] + m[2] * x[2])) / m[0];
}

// Sim3::log (sim3.h:148-230): omega, upsilon, sigma.  Returns the branch taken:
// bit 1 set when |sigma| >= eps, bit 0 set when d <= 1 - eps (acos is used).
__device__ inline int sim3_log(const double a[8], double out[7])
{
    const double s = a[7];
    const double sigma = log(s);
    double R[9];
    qmat(Q{a[0], a[1], a[2], a[3]}, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};   // deltaR (se3_ops.hpp:40-47)
    const double eps = 0.00001;
    double om[3], A, B, C;
    int branch;
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) {
#pragma unroll
            for (int i = 0; i < 3; i++) om[i] = 0.5 * dR[i];
            A = 1. / 2.;
            B = 1. / 6.;
            branch = 0;
        } else {
            const double theta = acos(d);
            const double theta2 = theta * theta;
            const double f = theta / (2 * sqrt(1 - d * d));
#pragma unroll
            for (int i = 0; i < 3; i++) om[i] = f * dR[i];
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
            branch = 1;
        }
    } else {
        C = (s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
#pragma unroll
            for (int i = 0; i < 3; i++) om[i] = 0.5 * dR[i];
            A = ((sigma - 1) * s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
            branch = 2;
        } else {
            const double theta = acos(d);
            const double f = theta / (2 * sqrt(1 - d * d));
#pragma unroll
            for (int i = 0; i < 3; i++) om[i] = f * dR[i];
            const double theta2 = theta * theta;
            const double sa = s * sin(theta);
            const double sb = s * cos(theta);
            const double c = theta2 + sigma * sigma;
            A = (sa * sigma + (1 - sb) * theta) / (theta * c);
            B = (C - ((sb - 1) * sigma + sa * theta) / (c)) * 1. / (theta2);
            branch = 3;
        }
    }
    // W = A * Omega + B * Omega * Omega + C * I, the middle term as (B * Omega) * Omega
    const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    double W[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double bo2 = (B * O[i * 3]) * O[j] + (B * O[i * 3 + 1]) * O[3 + j] + (B * O[i * 3 + 2]) * O[6 + j];
            W[i * 3 + j] = A * O[i * 3 + j] + bo2 + C * (i == j ? 1.0 : 0.0);
        }
    const double t[3] = {a[4], a[5], a[6]};
    double ups[3];
    lu3_solve(W, t, ups);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        out[i] = om[i];
        out[3 + i] = ups[i];
    }
    out[6] = sigma;
    return branch;
}

}  // namespace orbx
