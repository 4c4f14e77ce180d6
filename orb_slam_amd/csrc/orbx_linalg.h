// Small dense FP64 linear algebra shared by the initialisation models
// (orbx_init.hip), the new map points (orbx_newpoints.hip) and the
// reconstruction (orbx_reconstruct.hip): the defined 3x3 product and inverse
// and the 4x4 null vector.  Like orbx_jacobi.h, the
// text of these functions fixes the bits of every result that uses them.
#pragma once

#include "orbx_jacobi.h"

namespace orbx {

// Defined 3x3 arithmetic: FP64 from the float entries, rounded once.
// tests/init_numpy.py restates both in the same order.
__device__ inline void mul3(const float* a, const float* b, float* out)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double acc = (double)a[3 * i] * (double)b[j];
            acc = acc + (double)a[3 * i + 1] * (double)b[3 + j];
            acc = acc + (double)a[3 * i + 2] * (double)b[6 + j];
            out[3 * i + j] = (float)acc;
        }
}

__device__ inline void inv3(const float* mf, float* out)
{
    double m[9];
#pragma unroll
    for (int i = 0; i < 9; i++) m[i] = (double)mf[i];
    double c[9];
    c[0] = m[4] * m[8] - m[5] * m[7];
    c[1] = m[2] * m[7] - m[1] * m[8];
    c[2] = m[1] * m[5] - m[2] * m[4];
    c[3] = m[5] * m[6] - m[3] * m[8];
    c[4] = m[0] * m[8] - m[2] * m[6];
    c[5] = m[2] * m[3] - m[0] * m[5];
    c[6] = m[3] * m[7] - m[4] * m[6];
    c[7] = m[1] * m[6] - m[0] * m[7];
    c[8] = m[0] * m[4] - m[1] * m[3];
    const double det = (m[0] * c[0] + m[1] * c[3]) + m[2] * c[6];
#pragma unroll
    for (int i = 0; i < 9; i++) out[i] = (float)(c[i] / det);
}

// The unit right singular vector of A (row-major 4x4) for its smallest
// singular value: FP64 from the float entries, rounded once; sign unspecified.
__device__ inline void null_vector4(const float* A, float* out)
{
    double a[4][4], v[4][4];   // [column][row]
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            a[j][i] = (double)A[4 * i + j];
            v[j][i] = i == j ? 1.0 : 0.0;
        }
    double floor = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) floor += (a[j][0] * a[j][0] + a[j][1] * a[j][1]) + (a[j][2] * a[j][2] + a[j][3] * a[j][3]);
    floor *= kInitFloor;
    for (int sweep = 0; sweep < kInitSweeps; sweep++) {
        bool rot = false;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                const double al = (a[p][0] * a[p][0] + a[p][1] * a[p][1]) + (a[p][2] * a[p][2] + a[p][3] * a[p][3]);
                const double be = (a[q][0] * a[q][0] + a[q][1] * a[q][1]) + (a[q][2] * a[q][2] + a[q][3] * a[q][3]);
                const double ga = (a[p][0] * a[q][0] + a[p][1] * a[q][1]) + (a[p][2] * a[q][2] + a[p][3] * a[q][3]);
                if (jacobi_wants(al, be, ga, floor)) {
                    rot = true;
                    double c, s;
                    jacobi_cs(al, be, ga, c, s);
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const double ap = a[p][i], aq = a[q][i];
                        a[p][i] = c * ap - s * aq;
                        a[q][i] = s * ap + c * aq;
                        const double vp = v[p][i], vq = v[q][i];
                        v[p][i] = c * vp - s * vq;
                        v[q][i] = s * vp + c * vq;
                    }
                }
            }
        if (!rot) break;
    }
    double best = 0.0, nv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const double nj = (a[j][0] * a[j][0] + a[j][1] * a[j][1]) + (a[j][2] * a[j][2] + a[j][3] * a[j][3]);
        if (j == 0 || nj < best) {
            best = nj;
#pragma unroll
            for (int i = 0; i < 4; i++) nv[i] = v[j][i];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = (float)nv[i];
}

}  // namespace orbx
