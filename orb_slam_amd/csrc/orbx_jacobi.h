// FP64 Jacobi, the one text of it: the rotation tests and the rotation angle
// of both kinds (one-sided on a column pair's Gram entries, two-sided on a
// symmetric matrix' entries), and the one-sided (Hestenes) solve of a small
// matrix held in registers.  Users:
//   hestenes          null_vector4 (orbx_linalg.h: the triangulations of
//                     orbx_newpoints.hip and orbx_reconstruct.hip), svd3
//                     (orbx_reconstruct.hip), rank2_3x3 (orbx_init.hip)
//   jacobi_wants/_cs  hestenes, k_init_solve's 16-lane row form
//                     (orbx_init.hip), svd_cols (orbx_pnp.hip)
//   sym_wants/_cs     top_eigenvector4 (orbx_sim3.hip), sym_eig (orbx_pnp.hip)
// The text of these functions fixes the bits of every solve that uses them
// (DESIGN.md section 4).
#pragma once

#include <hip/hip_runtime.h>

namespace orbx {

constexpr int kInitSweeps = 40;            // Jacobi sweep cap (convergence takes 6-9)
constexpr double kInitTol = 8.9e-16;       // 4 eps: rotation threshold on |a_p . a_q| / (|a_p| |a_q|)

// Reciprocal and reciprocal square root from the hardware estimates and two
// Newton steps: a few units of FP64 round-off, which is all a Jacobi rotation
// needs (c^2 + s^2 = 1 to round-off keeps V orthogonal; the angle's error
// only leaves a smaller off-diagonal for the next sweep).  With the IEEE
// divide and square root sequences in their place the solve took 1.5 times
// as long.
__device__ inline double fast_rcp(double x)
{
    double y = __builtin_amdgcn_rcp(x);
    y = fma(fma(-x, y, 1.0), y, y);
    y = fma(fma(-x, y, 1.0), y, y);
    return y;
}

__device__ inline double fast_rsq(double x)
{
    double y = __builtin_amdgcn_rsq(x);
    const double h = 0.5 * x;
    y = fma(fma(-(h * y), y, 0.5), y, y);
    y = fma(fma(-(h * y), y, 0.5), y, y);
    return y;
}

// Whether columns with Gram entries al, be, ga still want a rotation:
// |ga| > kInitTol sqrt(al be), and neither column is below round-off of the
// whole matrix (floor = (eps |A|_F)^2).  A column that small is a null vector
// to FP64 backward error already; its products with the others are noise that
// never settles, and without the floor every 8x9 system -- which always has
// such a column -- ran to the sweep cap (40 sweeps where 7 converge).
__device__ inline bool jacobi_wants(double al, double be, double ga, double floor)
{
    return ga != 0.0 && ga * ga > (kInitTol * kInitTol) * (al * be) && al >= floor && be >= floor;
}
constexpr double kInitFloor = 4.93e-32;   // eps^2

// The two-sided test on the off-diagonal entry apq of a symmetric matrix:
// floor = kInitTol^2 |A|_F^2, so entries below 4 eps |A|_F are left.
__device__ inline bool sym_wants(double apq, double floor) { return apq != 0.0 && apq * apq > floor; }

// The rotation that annihilates ga: of columns p, q with Gram entries al, be,
// ga (one-sided), or of the symmetric entries app, aqq, apq (two-sided, which
// also moves the diagonal by t apq).
struct JacobiRot {
    double c, s, t;
};

__device__ inline JacobiRot jacobi_cs(double al, double be, double ga)
{
    double zeta = (be - al) * fast_rcp(2.0 * ga);
    zeta = fmin(fmax(zeta, -1e100), 1e100);   // a negligible ga: the identity, without inf - inf
    const double w = 1.0 + zeta * zeta;
    JacobiRot r;
    r.t = copysign(fast_rcp(fabs(zeta) + w * fast_rsq(w)), zeta);
    r.c = fast_rsq(1.0 + r.t * r.t);
    r.s = r.c * r.t;
    return r;
}

// An N x N matrix and the rotations applied to it, in registers,
// [column][row].  Passed and returned by value: reached by reference the
// arrays cost k_triangulate 32 VGPRs and a wave of occupancy.  Square only,
// and v before a: a rectangular form (a loop each for a's and v's rows) or the
// other member order schedules k_triangulate's rotations differently from the
// hand-written solve it replaced ("One Jacobi core, one defined
// arithmetic").
template <int N>
struct JacobiCols {
    double v[N][N], a[N][N];
};

// Columns of a row-major float matrix, V = I.
template <int N>
__device__ inline JacobiCols<N> load_cols(const float* A)
{
    JacobiCols<N> m;
#pragma unroll
    for (int j = 0; j < N; j++)
#pragma unroll
        for (int i = 0; i < N; i++) {
            m.a[j][i] = (double)A[N * i + j];
            m.v[j][i] = i == j ? 1.0 : 0.0;
        }
    return m;
}

// The summation order of a column dot product, per size: left to right at 3,
// pairwise at 4.
__device__ inline double col_dot(const double (&x)[3], const double (&y)[3])
{
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2];
}

__device__ inline double col_dot(const double (&x)[4], const double (&y)[4])
{
    return (x[0] * y[0] + x[1] * y[1]) + (x[2] * y[2] + x[3] * y[3]);
}

// One-sided Jacobi on the columns of m.a: on return column j is u_j sigma_j
// (unsorted) and m.v[j] the right singular vector j.  A NaN rotates nothing.
template <int N>
__device__ inline JacobiCols<N> hestenes(JacobiCols<N> m)
{
    double floor = 0.0;
#pragma unroll
    for (int j = 0; j < N; j++) floor += col_dot(m.a[j], m.a[j]);
    floor *= kInitFloor;
    for (int sweep = 0; sweep < kInitSweeps; sweep++) {
        bool rot = false;
#pragma unroll
        for (int p = 0; p < N - 1; p++)
#pragma unroll
            for (int q = p + 1; q < N; q++) {
                const double al = col_dot(m.a[p], m.a[p]);
                const double be = col_dot(m.a[q], m.a[q]);
                const double ga = col_dot(m.a[p], m.a[q]);
                if (jacobi_wants(al, be, ga, floor)) {
                    rot = true;
                    const JacobiRot r = jacobi_cs(al, be, ga);
#pragma unroll
                    for (int i = 0; i < N; i++) {
                        const double ap = m.a[p][i], aq = m.a[q][i];
                        m.a[p][i] = r.c * ap - r.s * aq;
                        m.a[q][i] = r.s * ap + r.c * aq;
                        const double vp = m.v[p][i], vq = m.v[q][i];
                        m.v[p][i] = r.c * vp - r.s * vq;
                        m.v[q][i] = r.s * vp + r.c * vq;
                    }
                }
            }
        if (!rot) break;
    }
    return m;
}

}  // namespace orbx
