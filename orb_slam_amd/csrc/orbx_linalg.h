// The defined arithmetic of the geometry solvers, the one text of it
// (DESIGN.md section 4): the "float gemm" -- FP64 accumulation over k in
// order, rounded once -- with the products, norm and affine map built on it,
// the 3x3 adjugate (inverse and determinant), the 4x4 null vector and the
// reprojection error.  Users: orbx_init.hip (mul3, inv3), orbx_reconstruct.hip
// (all of it), orbx_newpoints.hip (dot3, tmatvec3, affine3, norm3,
// null_vector4, reproj_e2), orbx_sim3.hip (dot3, affine3, norm3).  Like
// orbx_jacobi.h, the text of these functions fixes the bits of every result
// that uses them.
#pragma once

#include "orbx_jacobi.h"

namespace orbx {

// The defined float gemm: FP64 accumulation over k in order (rounded by the
// caller, after the addend or the scalar where there is one).  A product of
// two floats is exact in FP64, so only the order of the sum is part of the
// definition.  tests/init_numpy.py restates it in the same order.
__device__ inline double dot3(const float* r, float x0, float x1, float x2)
{
    double acc = (double)r[0] * (double)x0;
    acc = acc + (double)r[1] * (double)x1;
    acc = acc + (double)r[2] * (double)x2;
    return acc;
}

__device__ inline double dot3(const float* r, const float* x) { return dot3(r, x[0], x[1], x[2]); }

// a * b and (s * a) * b of row-major 3x3 (the scale before the rounding)
__device__ inline void mul3(const float* a, const float* b, float* out)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) out[3 * i + j] = (float)dot3(a + 3 * i, b[j], b[3 + j], b[6 + j]);
}

__device__ inline void scaled_mul3(float s, const float* a, const float* b, float* out)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) out[3 * i + j] = (float)((double)s * dot3(a + 3 * i, b[j], b[3 + j], b[6 + j]));
}

// m * v and m.t() * v
__device__ inline void matvec3(const float* m, const float* v, float* out)
{
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = (float)dot3(m + 3 * i, v);
}

__device__ inline void tmatvec3(const float* m, const float* v, float* out)
{
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = (float)dot3(v, m[i], m[3 + i], m[6 + i]);
}

// row . x + t: the float addend joins the double sum, the assignment rounds
__device__ inline float affine3(const float* row, const float* x, float t) { return (float)(dot3(row, x) + (double)t); }

__device__ inline double norm3(const float* x) { return sqrt(dot3(x, x)); }

// The cofactors of a float 3x3 in FP64, laid out as the adjugate (row-major);
// returns the determinant, expanded along the first row.
__device__ inline double adj3(const float* mf, double* c)
{
    double m[9];
#pragma unroll
    for (int i = 0; i < 9; i++) m[i] = (double)mf[i];
    c[0] = m[4] * m[8] - m[5] * m[7];
    c[1] = m[2] * m[7] - m[1] * m[8];
    c[2] = m[1] * m[5] - m[2] * m[4];
    c[3] = m[5] * m[6] - m[3] * m[8];
    c[4] = m[0] * m[8] - m[2] * m[6];
    c[5] = m[2] * m[3] - m[0] * m[5];
    c[6] = m[3] * m[7] - m[4] * m[6];
    c[7] = m[1] * m[6] - m[0] * m[7];
    c[8] = m[0] * m[4] - m[1] * m[3];
    return (m[0] * c[0] + m[1] * c[3]) + m[2] * c[6];
}

__device__ inline void inv3(const float* mf, float* out)
{
    double c[9];
    const double det = adj3(mf, c);
#pragma unroll
    for (int i = 0; i < 9; i++) out[i] = (float)(c[i] / det);
}

// cv::determinant of a 3x3 float matrix
__device__ inline double det3(const float* mf)
{
    double c[9];
    return adj3(mf, c);
}

// The unit right singular vector of A (row-major 4x4) for its smallest
// singular value: FP64 from the float entries, rounded once; sign unspecified.
__device__ inline void null_vector4(const float* A, float* out)
{
    const JacobiCols<4> m = hestenes(load_cols<4>(A));
    double best = 0.0, nv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const double nj = col_dot(m.a[j], m.a[j]);
        if (j == 0 || nj < best) {
            best = nj;
#pragma unroll
            for (int i = 0; i < 4; i++) nv[i] = m.v[j][i];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = (float)nv[i];
}

// Squared reprojection error of the camera point (x, y, z) against the pixel
// (u, v), the reference's float source: follows orbx_set_fp_contract.  The
// caller compares it with its own threshold.  (Sim3's cam_to_image is another
// arithmetic: it divides in float and multiplies x by 1/z before f.)
__device__ inline float reproj_e2(const float* cam, float x, float y, float z, float u, float v, int contract)
{
    const float invz = (float)(1.0 / (double)z);
    float imx, imy;
    if (contract) {
        imx = fmaf(cam[0] * x, invz, cam[2]);
        imy = fmaf(cam[1] * y, invz, cam[3]);
    } else {
        imx = cam[0] * x * invz + cam[2];
        imy = cam[1] * y * invz + cam[3];
    }
    const float ex = imx - u, ey = imy - v;
    return contract ? fmaf(ex, ex, ey * ey) : ex * ex + ey * ey;
}

}  // namespace orbx
