// One-sided (Hestenes) Jacobi in FP64: the rotation test and the rotation of
// a column pair, shared by the null-vector solves of the initialisation
// models (orbx_init.hip, 16x9 and 3x3) and of the triangulation
// (orbx_newpoints.hip, 4x4).  The text of these functions fixes the bits of
// every solve that uses them.
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

// Hestenes rotation of columns p, q with Gram entries al, be, ga.
__device__ inline void jacobi_cs(double al, double be, double ga, double& c, double& s)
{
    double zeta = (be - al) * fast_rcp(2.0 * ga);
    zeta = fmin(fmax(zeta, -1e100), 1e100);   // a negligible ga: the identity, without inf - inf
    const double w = 1.0 + zeta * zeta;
    const double t = copysign(fast_rcp(fabs(zeta) + w * fast_rsq(w)), zeta);
    c = fast_rsq(1.0 + t * t);
    s = c * t;
}

}  // namespace orbx
