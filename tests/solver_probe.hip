// Test-only probe of the solvers' shared device headers (orbx_lm.h,
// orbx_jacobi.h, orbx_linalg.h, orbx_se3.h, orbx_sim3_dev.h): one kernel per
// probed function, one thread per input, never linked into liborbx.so.
// tests/solver_probe.py builds it with the library's compiler and flags and
// launches it through ctypes.
//
// Every record is an array of doubles: NI per item in, NO per item out.  The
// float functions get their arguments narrowed from doubles that hold floats
// (exact both ways), and flags and branch numbers come back as 0.0, 1.0, ...
// A kernel indexes memory by its item index only, never by data, so NaN,
// infinity, zero and denormal inputs are arithmetic and nothing else.
#include <hip/hip_runtime.h>

#include "orbx_linalg.h"
#include "orbx_lm.h"
#include "orbx_sim3_dev.h"

using namespace orbx;

namespace {

typedef void (*probe_kernel)(int, const double*, double*);

int launch(probe_kernel k, int n, int ni, int no, const void* in, void* out)
{
    if (n <= 0) return 0;
    double *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&din, sizeof(double) * n * ni);
    if (e == hipSuccess) e = hipMalloc(&dout, sizeof(double) * n * no);
    if (e == hipSuccess) e = hipMemcpy(din, in, sizeof(double) * n * ni, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0xff, sizeof(double) * n * no);
    if (e == hipSuccess) {
        k<<<(n + 63) / 64, 64>>>(n, din, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, sizeof(double) * n * no, hipMemcpyDeviceToHost);
    (void)hipFree(din);
    (void)hipFree(dout);
    return (int)e;
}

template <int N>
__device__ void to_float(const double* a, float (&f)[N])
{
#pragma unroll
    for (int k = 0; k < N; k++) f[k] = (float)a[k];
}

}  // namespace

// body: __device__ void(const double (&a)[NI], double (&o)[NO])
#define PROBE(name, NI, NO)                                                              \
    __global__ void k_##name(int n, const double* in, double* out)                       \
    {                                                                                    \
        const int i = blockIdx.x * 64 + threadIdx.x;                                     \
        if (i >= n) return;                                                              \
        double a[NI], o[NO];                                                             \
        _Pragma("unroll") for (int k = 0; k < NI; k++) a[k] = in[(size_t)i * NI + k];    \
        body_##name(a, o);                                                               \
        _Pragma("unroll") for (int k = 0; k < NO; k++) out[(size_t)i * NO + k] = o[k];   \
    }                                                                                    \
    extern "C" int probe_##name(int n, const void* in, void* out) { return launch(k_##name, n, NI, NO, in, out); }

// --- orbx_lm.h -----------------------------------------------------------------------
template <int N>
__device__ void body_ldlt(const double* a, double* o)
{
    constexpr int P = N * (N + 1) / 2;
    double m[P], b[N], x[N];
#pragma unroll
    for (int k = 0; k < P; k++) m[k] = a[k];
#pragma unroll
    for (int k = 0; k < N; k++) b[k] = a[P + k];
    const bool ok = ldlt_solve<N>(m, b, x);
#pragma unroll
    for (int k = 0; k < N; k++) o[k] = x[k];
    o[N] = ok ? 1.0 : 0.0;
}

__device__ void body_ldlt6(const double (&a)[27], double (&o)[7]) { body_ldlt<6>(a, o); }
PROBE(ldlt6, 27, 7)

__device__ void body_ldlt7(const double (&a)[35], double (&o)[8]) { body_ldlt<7>(a, o); }
PROBE(ldlt7, 35, 8)

__device__ void body_huber(const double (&a)[2], double (&o)[2]) { huber(a[0], a[1], o[0], o[1]); }
PROBE(huber, 2, 2)

// lambda, ni, nBad, currentChi, tempChi, ok, scale -> lambda, ni, nBad, currentChi, accept, rho
__device__ void body_lm_trial(const double (&a)[7], double (&o)[6])
{
    LmState s{a[0], a[1], (int)a[2]};
    double chi = a[3];
    const LmTrial t = lm_trial(s, chi, a[4], a[5] != 0.0, a[6]);
    o[0] = s.lambda;
    o[1] = s.ni;
    o[2] = (double)s.nBad;
    o[3] = chi;
    o[4] = t.accept ? 1.0 : 0.0;
    o[5] = t.rho;
}
PROBE(lm_trial, 7, 6)

__device__ void body_lm_retry(const double (&a)[2], double (&o)[1]) { o[0] = lm_retry(a[0], (int)a[1]) ? 1.0 : 0.0; }
PROBE(lm_retry, 2, 1)

// nBad, qmax, rho, iniChi, currentChi -> stop, nBad
__device__ void body_lm_stop(const double (&a)[5], double (&o)[2])
{
    LmState s{0.0, 2.0, (int)a[0]};
    o[0] = lm_stop(s, (int)a[1], a[2], a[3], a[4]) ? 1.0 : 0.0;
    o[1] = (double)s.nBad;
}
PROBE(lm_stop, 5, 2)

// x[7], lambda, b[7] -> scale
__device__ void body_lm_scale7(const double (&a)[15], double (&o)[1])
{
    double x[7], b[7];
#pragma unroll
    for (int k = 0; k < 7; k++) {
        x[k] = a[k];
        b[k] = a[8 + k];
    }
    o[0] = lm_scale<7>(x, a[7], b);
}
PROBE(lm_scale7, 15, 1)

// --- orbx_jacobi.h -------------------------------------------------------------------
__device__ void body_rcp(const double (&a)[1], double (&o)[1]) { o[0] = fast_rcp(a[0]); }
PROBE(rcp, 1, 1)

__device__ void body_rsq(const double (&a)[1], double (&o)[1]) { o[0] = fast_rsq(a[0]); }
PROBE(rsq, 1, 1)

__device__ void body_jacobi_wants(const double (&a)[4], double (&o)[1]) { o[0] = jacobi_wants(a[0], a[1], a[2], a[3]) ? 1.0 : 0.0; }
PROBE(jacobi_wants, 4, 1)

__device__ void body_sym_wants(const double (&a)[2], double (&o)[1]) { o[0] = sym_wants(a[0], a[1]) ? 1.0 : 0.0; }
PROBE(sym_wants, 2, 1)

__device__ void body_jacobi_cs(const double (&a)[3], double (&o)[3])
{
    const JacobiRot r = jacobi_cs(a[0], a[1], a[2]);
    o[0] = r.c;
    o[1] = r.s;
    o[2] = r.t;
}
PROBE(jacobi_cs, 3, 3)

// row-major floats -> a[col][row], then v[col][row]
template <int N>
__device__ void body_hestenes(const double* a, double* o)
{
    float A[N * N];
    to_float(a, A);
    const JacobiCols<N> m = hestenes(load_cols<N>(A));
#pragma unroll
    for (int j = 0; j < N; j++)
#pragma unroll
        for (int i = 0; i < N; i++) {
            o[N * j + i] = m.a[j][i];
            o[N * N + N * j + i] = m.v[j][i];
        }
}

__device__ void body_hestenes3(const double (&a)[9], double (&o)[18]) { body_hestenes<3>(a, o); }
PROBE(hestenes3, 9, 18)

__device__ void body_hestenes4(const double (&a)[16], double (&o)[32]) { body_hestenes<4>(a, o); }
PROBE(hestenes4, 16, 32)

// --- orbx_linalg.h -------------------------------------------------------------------
__device__ void body_null_vector4(const double (&a)[16], double (&o)[4])
{
    float A[16], v[4];
    to_float(a, A);
    null_vector4(A, v);
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = (double)v[k];
}
PROBE(null_vector4, 16, 4)

// a[9], b[9], v[3], s, t -> mul3 9, scaled_mul3 9, matvec3 3, tmatvec3 3, affine3 (row 0 of a), norm3(v), inv3(a) 9, det3(a)
__device__ void body_linalg3(const double (&a)[23], double (&o)[36])
{
    float f[23], r[9];
    to_float(a, f);
    const float *A = f, *B = f + 9, *v = f + 18;
    mul3(A, B, r);
#pragma unroll
    for (int k = 0; k < 9; k++) o[k] = (double)r[k];
    scaled_mul3(f[21], A, B, r);
#pragma unroll
    for (int k = 0; k < 9; k++) o[9 + k] = (double)r[k];
    matvec3(A, v, r);
#pragma unroll
    for (int k = 0; k < 3; k++) o[18 + k] = (double)r[k];
    tmatvec3(A, v, r);
#pragma unroll
    for (int k = 0; k < 3; k++) o[21 + k] = (double)r[k];
    o[24] = (double)affine3(A, v, f[22]);
    o[25] = norm3(v);
    inv3(A, r);
#pragma unroll
    for (int k = 0; k < 9; k++) o[26 + k] = (double)r[k];
    o[35] = det3(A);
}
PROBE(linalg3, 23, 36)

// cam[4], x, y, z, u, v -> e2 with contract 0, with contract 1
__device__ void body_reproj_e2(const double (&a)[9], double (&o)[2])
{
    float f[9];
    to_float(a, f);
    o[0] = (double)reproj_e2(f, f[4], f[5], f[6], f[7], f[8], 0);
    o[1] = (double)reproj_e2(f, f[4], f[5], f[6], f[7], f[8], 1);
}
PROBE(reproj_e2, 9, 2)

// --- orbx_se3.h ----------------------------------------------------------------------
// m[9], q1, q2, v[3] -> qfrom(m) 4, qmat(q1) 9, qmul(q1, q2) 4, qrot(q1, v) 3, qnormalize(q1) 4
__device__ void body_quat(const double (&a)[20], double (&o)[24])
{
    double m[9], v[3], r[3];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = a[k];
    const Q q1{a[9], a[10], a[11], a[12]}, q2{a[13], a[14], a[15], a[16]};
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = a[17 + k];
    const Q f = qfrom(m);
    o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = f.w;
    double R[9];
    qmat(q1, R);
#pragma unroll
    for (int k = 0; k < 9; k++) o[4 + k] = R[k];
    const Q p = qmul(q1, q2);
    o[13] = p.x; o[14] = p.y; o[15] = p.z; o[16] = p.w;
    qrot(q1, v, r);
#pragma unroll
    for (int k = 0; k < 3; k++) o[17 + k] = r[k];
    Q nq = q1;
    qnormalize(nq);
    o[20] = nq.x; o[21] = nq.y; o[22] = nq.z; o[23] = nq.w;
}
PROBE(quat, 20, 24)

// pose[7], u[6] -> pose[7]
__device__ void body_se3_oplus(const double (&a)[13], double (&o)[7])
{
    double pose[7], u[6];
#pragma unroll
    for (int k = 0; k < 7; k++) pose[k] = a[k];
#pragma unroll
    for (int k = 0; k < 6; k++) u[k] = a[7 + k];
    se3_oplus(pose, u);
#pragma unroll
    for (int k = 0; k < 7; k++) o[k] = pose[k];
}
PROBE(se3_oplus, 13, 7)

// pose[7], p[3] -> o[3]
__device__ void body_se3_map(const double (&a)[10], double (&o)[3])
{
    double pose[7], p[3];
#pragma unroll
    for (int k = 0; k < 7; k++) pose[k] = a[k];
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = a[7 + k];
    se3_map(pose, p, o);
}
PROBE(se3_map, 10, 3)

// --- orbx_sim3_dev.h -----------------------------------------------------------------
// u[7], es -> Sim3[8]
__device__ void body_sim3_exp(const double (&a)[8], double (&o)[8])
{
    double u[7];
#pragma unroll
    for (int k = 0; k < 7; k++) u[k] = a[k];
    sim3_exp(u, a[7], o);
}
PROBE(sim3_exp, 8, 8)

__device__ void body_sim3_mul(const double (&a)[16], double (&o)[8])
{
    double x[8], y[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        x[k] = a[k];
        y[k] = a[8 + k];
    }
    sim3_mul(x, y, o);
}
PROBE(sim3_mul, 16, 8)

__device__ void body_sim3_inverse(const double (&a)[8], double (&o)[8])
{
    double x[8];
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = a[k];
    sim3_inverse(x, o);
}
PROBE(sim3_inverse, 8, 8)

__device__ void body_sim3_map(const double (&a)[11], double (&o)[3])
{
    double x[8], p[3];
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = a[k];
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = a[8 + k];
    sim3_map(x, p, o);
}
PROBE(sim3_map, 11, 3)

// m[9] row-major, b[3] -> x[3]
__device__ void body_lu3(const double (&a)[12], double (&o)[3])
{
    double m[9], b[3];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = a[k];
#pragma unroll
    for (int k = 0; k < 3; k++) b[k] = a[9 + k];
    lu3_solve(m, b, o);
}
PROBE(lu3, 12, 3)

// Sim3[8] -> log[7], branch
__device__ void body_sim3_log(const double (&a)[8], double (&o)[8])
{
    double x[8], l[7];
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = a[k];
    const int br = sim3_log(x, l);
#pragma unroll
    for (int k = 0; k < 7; k++) o[k] = l[k];
    o[7] = (double)br;
}
PROBE(sim3_log, 8, 8)
