// PnPsolver on the device (src/PnPsolver.cc): the constructor, and one
// PnPsolver::iterate call with every RANSAC iteration the call can run
// evaluated at once from the caller's rand() draws.
//
// Five kernels per call, each over all candidates of the call:
//   k_pnp_prepare  a workgroup per candidate: wave 0 walks the keypoints in
//                  order and keeps the correspondences (ballot prefix); then a
//                  thread per iteration draws its minimal set of four.
//   k_pnp_solve    EPnP, sixteen lanes per hypothesis and four hypotheses per
//                  wave, the matrices in LDS: the 12x12 Gram matrix a few
//                  entries per lane, its eigenvectors by a two-sided FP64
//                  Jacobi with a lane per row, the three beta sets a lane each.
//   k_pnp_check    a workgroup per candidate: the correspondences staged in
//                  LDS tiles, a lane per (iteration, slice), integer counts
//                  summed with LDS atomics; then thread 0 lists the strict
//                  record holders among the iterations with count >= min.
//   k_pnp_refine   Refine of the incoming best set and of every record
//                  holder: the inlier set recomputed and compacted, EPnP over
//                  it (the same code, the sums over the points sequential in
//                  their order), CheckInliers of the refit.
//   k_pnp_select   thread 0 replays iterate's loop over the counts and the
//                  refits' counts; the workgroup writes the returned mask and
//                  the best-set state.
//
// What the reference writes itself is followed operation by operation (this
// file is compiled without contraction; CheckInliers' expressions fuse
// explicitly under orbx_set_fp_contract); the five places that go through
// OpenCV are the definitions of DESIGN.md section 4 (tests/pnp_numpy.py
// restates the rest and takes those from the taps).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "orbx_bow_queue.h"
#include "orbx_device.h"
#include "orbx_internal.h"
#include "orbx_jacobi.h"
#include "orbx_stage.h"

namespace orbx {

constexpr int kPnpMaxIter = 1024;
constexpr int kPnpTile = 1024;     // correspondences staged per LDS tile of k_pnp_check
constexpr int kPnpFloats = 6;      // per staged correspondence
constexpr int kPnpLanes = 16;      // lanes per hypothesis
constexpr int kPnpGroups = 4;      // hypotheses per wave
constexpr int kPnpRefineBlocks = 8;
constexpr int kRec = ORBX_PNP_REC;
// offsets inside a hypothesis record (doubles)
constexpr int R_DC = 0, R_UCT = 3, R_CI = 12, R_UT = 21, R_B = 69, R_UV = 81, R_L = 135, R_RHO = 195, R_BETAS = 201,
              R_R = 213, R_T = 222, R_ERR = 225, R_CHOSEN = 228, R_NPTS = 229;

struct PnpHdr {
    int32_t N, min_inl, max_its, E, run, discarded, n_rec, iters_run;
    int32_t no_more, found, found_iter, n_inliers, refined, best_out, best_slot, iter_out;
    float Tcw[16];
    float best_Tcw[16];
};

// One candidate: device pointers to its inputs and the solver's state.
struct PnpCand {
    const orbx_keypoint* keys;   // the frame's
    const int32_t* match;        // slot form: per frame keypoint the keyframe's keypoint, else null
    const uint8_t* valid;        // host forms: per frame keypoint; slot form: per keyframe keypoint (1 = map point)
    const float* pos;            // host forms: per frame keypoint; slot form: per keyframe keypoint
    const float* sigma2;
    const int32_t* draws;
    const uint8_t* mask_in;      // per frame keypoint
    const int32_t* tab_min;      // mRansacMinInliers / mRansacMaxIts by N (slot form), else null
    const int32_t* tab_its;
    const int32_t* n_matches;    // the search's count (slot form), or null
    int32_t n, n2, nlevels, min_inl, max_its, min_matches, iter_done, best_in, n_iter, n_draws;
    float th2;
    float cam[4];
    float Tcw_in[16];
};

// Byte offsets inside one candidate's result block.
struct PnpLayout {
    long long stride;
    long long o_kp, o_p2, o_p3, o_me, o_sets, o_rec, o_cnt, o_recl, o_rrec, o_rcnt, o_ridx, o_inl, o_mask;
    int M, K, cap, head;
};

inline PnpLayout pnp_layout(int M, int cap)
{
    PnpLayout L;
    BlockOffsets o;
    L.M = M;
    L.cap = cap;
    L.K = std::min(M, cap) + 1;
    o.take(sizeof(PnpHdr));
    L.o_inl = o.take(cap);
    L.o_mask = o.take(cap);
    L.head = (int)o.end;   // what a call without taps reads back
    L.o_kp = o.take((long long)cap * 4);
    L.o_p2 = o.take((long long)cap * 8);
    L.o_p3 = o.take((long long)cap * 12);
    L.o_me = o.take((long long)cap * 4);
    L.o_sets = o.take((long long)M * 16);
    L.o_rec = o.take((long long)M * kRec * 8);
    L.o_cnt = o.take((long long)M * 4);
    L.o_recl = o.take((long long)L.K * 4);
    L.o_rrec = o.take((long long)L.K * kRec * 8);
    L.o_rcnt = o.take((long long)L.K * 4);
    L.o_ridx = o.take((long long)kPnpRefineBlocks * cap * 4);
    L.stride = o.end;
    return L;
}

// ---------------------------------------------------------------------------
// k_pnp_prepare
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pnp_prepare(const PnpCand* __restrict__ cands, uint8_t* __restrict__ res,
                                                     PnpLayout L)
{
    __shared__ int s_n;
    const PnpCand& d = cands[blockIdx.x];
    uint8_t* blk = res + (long long)blockIdx.x * L.stride;
    PnpHdr* hdr = reinterpret_cast<PnpHdr*>(blk);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = max(0, min(d.n, L.cap));
    const bool discarded = d.n_matches && *d.n_matches < d.min_matches;

    if (wave == 0) {
        int32_t* kp = reinterpret_cast<int32_t*>(blk + L.o_kp);
        float* p2 = reinterpret_cast<float*>(blk + L.o_p2);
        float* p3 = reinterpret_cast<float*>(blk + L.o_p3);
        float* me = reinterpret_cast<float*>(blk + L.o_me);
        const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
        int base = 0;
        for (int c = 0; c < n && !discarded; c += 64) {
            const int i = c + lane;
            int src = -1, oct = 0;
            bool ok = false;
            if (i < n) {
                if (d.match) {
                    src = d.match[i];
                    ok = src >= 0 && src < d.n2 && d.valid[src] == 1;
                } else {
                    src = i;
                    ok = d.valid[i] != 0;
                }
                if (ok) {
                    oct = d.keys[i].octave;
                    ok = oct >= 0 && oct < d.nlevels;
                }
            }
            const unsigned long long bal = __ballot(ok);
            if (ok) {
                const int at = base + __popcll(bal & lt_mask);   // < n <= cap
                kp[at] = i;
                p2[2 * at] = d.keys[i].x;
                p2[2 * at + 1] = d.keys[i].y;
                p3[3 * at] = d.pos[3 * src];
                p3[3 * at + 1] = d.pos[3 * src + 1];
                p3[3 * at + 2] = d.pos[3 * src + 2];
                me[at] = d.sigma2[oct] * d.th2;   // mvMaxError (:128)
            }
            base += __popcll(bal);
        }
        if (lane == 0) s_n = base;
    }
    __syncthreads();
    const int N = s_n;
    const int min_inl = d.tab_min ? d.tab_min[min(N, kMaxFeatures)] : d.min_inl;
    const int max_its = d.tab_its ? d.tab_its[min(N, kMaxFeatures)] : d.max_its;
    const bool run = !discarded && N >= min_inl && N >= 4;
    // the loop's condition is an or (:154)
    const int E = run ? min(max(d.n_iter, max_its - d.iter_done), min(d.n_draws, L.M)) : 0;
    if (tid == 0) {
        hdr->N = N;
        hdr->min_inl = min_inl;
        hdr->max_its = max_its;
        hdr->discarded = discarded;
        hdr->run = run;
        hdr->E = E;
    }
    // the minimal sets (:160-173): vAvailableIndices is the identity but for
    // the places earlier picks of this iteration overwrote, kept as a list.
    // The removal writes at the drawn *value* (:171), so pos[] holds values.
    int32_t* sets = reinterpret_cast<int32_t*>(blk + L.o_sets);
    for (int it = tid; it < E; it += blockDim.x) {
        int pos[4], val[4];
        const int32_t* dr = d.draws + (long long)it * 4;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int size = N - j;
            const int randi = (int)(((double)dr[j] / 2147483648.0) * (double)size);
            int idx = randi;
            int back = size - 1;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < j) {
                    if (pos[k] == randi) idx = val[k];
                    if (pos[k] == size - 1) back = val[k];
                }
            pos[j] = idx;
            val[j] = back;
            sets[it * 4 + j] = idx;
        }
    }
}

// ---------------------------------------------------------------------------
// EPnP
// ---------------------------------------------------------------------------
// The LDS of one hypothesis.
struct EpnpBranch {
    double A[30], V[25], b[6], x[4], A1[4], A2[4], abt[9], av[9], R[9], t[3], err;
};
struct EpnpLds {
    double A[144], V[144];   // MtM, then its diagonal form; the eigenvectors as rows
    double ut[48];           // rows 8..11 of Ut
    double L[60], rho[6];
    double cws[12], ci[9];
    double g3[9], v3[9], cc[9], vc[9];
    EpnpBranch br[3];
};

// One-sided (Hestenes) Jacobi on the columns of the row-major m x n matrix A:
// on return column j is u_j * sigma_j and V[j*n + i] component i of the right
// singular vector j.  A NaN rotates nothing.
__device__ inline void svd_cols(double* A, int m, int n, double* V)
{
    double frob = 0.0;
    for (int i = 0; i < m * n; i++) frob += A[i] * A[i];
    const double floor = kInitFloor * frob;
    for (int j = 0; j < n; j++)
        for (int i = 0; i < n; i++) V[j * n + i] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kInitSweeps; sweep++) {
        bool rot = false;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                double al = 0.0, be = 0.0, ga = 0.0;   // from 0.0 over a run-time m: not col_dot's sums
                for (int i = 0; i < m; i++) {
                    const double ap = A[i * n + p], aq = A[i * n + q];
                    al += ap * ap;
                    be += aq * aq;
                    ga += ap * aq;
                }
                if (jacobi_wants(al, be, ga, floor)) {
                    rot = true;
                    const JacobiRot g = jacobi_cs(al, be, ga);
                    const double c = g.c, s = g.s;
                    for (int i = 0; i < m; i++) {
                        const double ap = A[i * n + p], aq = A[i * n + q];
                        A[i * n + p] = c * ap - s * aq;
                        A[i * n + q] = s * ap + c * aq;
                    }
                    for (int i = 0; i < n; i++) {
                        const double vp = V[p * n + i], vq = V[q * n + i];
                        V[p * n + i] = c * vp - s * vq;
                        V[q * n + i] = s * vp + c * vq;
                    }
                }
            }
        if (!rot) break;
    }
}

// Two-sided cyclic Jacobi on the symmetric n x n matrix A in LDS; V[j*n + k]
// ends as component k of the eigenvector of A[j*n + j].  Rotations below
// 4 eps |A|_F are left, so a null space keeps whatever basis the sweeps
// reached.  SYNC: the lanes of a group share the rows (lane, lane + nl, ...)
// and the whole wave walks the pairs together; a group that is not active
// rotates nothing.  Otherwise one lane does it all.
template <bool SYNC>
__device__ inline void sym_eig(double* A, double* V, int n, int lane, int nl, bool act)
{
    double frob = 0.0;
    if (act)
        for (int i = 0; i < n * n; i++) frob += A[i] * A[i];
    const double floor = (kInitTol * kInitTol) * frob;
    if (act)
        for (int k = lane; k < n; k += nl)
            for (int j = 0; j < n; j++) V[j * n + k] = j == k ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kInitSweeps; sweep++) {
        bool rot = false;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                if (SYNC) __syncthreads();
                double apq = 0.0, app = 0.0, aqq = 0.0;
                if (act) {
                    apq = A[p * n + q];
                    app = A[p * n + p];
                    aqq = A[q * n + q];
                }
                // act last: apq is 0.0 in an inactive group, and this order keeps the kernels' control flow
                if (sym_wants(apq, floor) && act) {
                    rot = true;
                    const JacobiRot g = jacobi_cs(app, aqq, apq);
                    const double c = g.c, s = g.s, t = g.t;
                    for (int k = lane; k < n; k += nl) {
                        const double vp = V[p * n + k], vq = V[q * n + k];
                        V[p * n + k] = c * vp - s * vq;
                        V[q * n + k] = s * vp + c * vq;
                        if (k == p) {
                            A[p * n + p] = app - t * apq;
                            A[p * n + q] = 0.0;
                        } else if (k == q) {
                            A[q * n + q] = aqq + t * apq;
                            A[q * n + p] = 0.0;
                        } else {
                            const double akp = A[k * n + p], akq = A[k * n + q];
                            const double np = c * akp - s * akq, nq = s * akp + c * akq;
                            A[k * n + p] = np;
                            A[p * n + k] = np;
                            A[k * n + q] = nq;
                            A[q * n + k] = nq;
                        }
                    }
                }
            }
        if (SYNC ? !__any(rot) : !rot) break;
    }
    if (SYNC) __syncthreads();
}

// The correspondences a hypothesis is computed from: idx[i] into p3 / p2.
struct EpnpPoints {
    const int32_t* idx;
    const float* p3;
    const float* p2;
    int n;
    __device__ double pw(int i, int j) const { return (double)p3[3 * idx[i] + j]; }
    __device__ double u(int i, int j) const { return (double)p2[2 * idx[i] + j]; }
};

// alphas of point i (:395-405)
__device__ inline void epnp_alphas(const EpnpPoints& P, int i, const double* cws, const double* ci, double* a)
{
    const double d0 = P.pw(i, 0) - cws[0], d1 = P.pw(i, 1) - cws[1], d2 = P.pw(i, 2) - cws[2];
#pragma unroll
    for (int j = 0; j < 3; j++) a[1 + j] = (ci[3 * j] * d0 + ci[3 * j + 1] * d1) + ci[3 * j + 2] * d2;
    a[0] = ((1.0 - a[1]) - a[2]) - a[3];
}

__device__ inline double sel4(const double* a, int j) { return j == 0 ? a[0] : j == 1 ? a[1] : j == 2 ? a[2] : a[3]; }

// Entry `col` of row 2i + parity of M (:408-423)
__device__ inline double epnp_m(const double* a, int parity, int col, double f0, double f1, double du, double dv)
{
    const int j = col / 3, k = col - 3 * j;
    const double aj = sel4(a, j);
    if (k == 2) return aj * (parity ? dv : du);
    if (k == parity) return aj * (parity ? f1 : f0);
    return 0.0;
}

// The pseudo-inverse weights of singular values (SVBkSb's cut-off)
__device__ inline double sv_inv(double w, double cut) { return w > cut ? 1.0 / w : 0.0; }

// One beta set after its cvSolve (:655-665, :686-697, :720-729), gauss_newton
// (:812-830) and compute_R_and_t (:623-634), by one lane on its own LDS.
__device__ inline void epnp_branch(int which, const EpnpPoints& P, EpnpLds& S, EpnpBranch& W, const double* camd,
                                   double* rec)
{
    const int n = P.n;
    const int nc = which == 1 ? 4 : which == 2 ? 3 : 5;
    // (d) cvSolve(CV_SVD): the minimum-norm least squares of L_6xk b = rho
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < nc; j++) {
            const int col = which == 1 ? (j == 0 ? 0 : j == 1 ? 1 : j == 2 ? 3 : 6) : j;
            W.A[i * nc + j] = S.L[10 * i + col];
        }
    svd_cols(W.A, 6, nc, W.V);
    double b[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    {
        double wsum = 0.0;
        for (int j = 0; j < nc; j++) {
            double w2 = 0.0;
            for (int i = 0; i < 6; i++) w2 += W.A[i * nc + j] * W.A[i * nc + j];
            W.b[j] = sqrt(w2);
            wsum += W.b[j];
        }
        const double cut = 2.0 * DBL_EPSILON * wsum;
        for (int j = 0; j < nc; j++) {
            const double wi = sv_inv(W.b[j], cut);
            double ub = 0.0;
            for (int i = 0; i < 6; i++) ub += (W.A[i * nc + j] * wi) * S.rho[i];
            const double coef = ub * wi;
#pragma unroll
            for (int k = 0; k < 5; k++)
                if (k < nc) b[k] += coef * W.V[j * nc + k];
        }
    }
    const int ob = which == 1 ? 0 : which == 2 ? 4 : 7;
#pragma unroll
    for (int k = 0; k < 5; k++)
        if (k < nc) rec[R_B + ob + k] = b[k];
    double be[4] = {0.0, 0.0, 0.0, 0.0};
    if (which == 1) {
        if (b[0] < 0) {
            be[0] = sqrt(-b[0]);
            be[1] = -b[1] / be[0];
            be[2] = -b[2] / be[0];
            be[3] = -b[3] / be[0];
        } else {
            be[0] = sqrt(b[0]);
            be[1] = b[1] / be[0];
            be[2] = b[2] / be[0];
            be[3] = b[3] / be[0];
        }
    } else {
        if (b[0] < 0) {
            be[0] = sqrt(-b[0]);
            be[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0;
        } else {
            be[0] = sqrt(b[0]);
            be[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0;
        }
        if (b[1] < 0) be[0] = -be[0];
        if (which == 3) be[2] = b[3] / be[0];
    }
    // gauss_newton: five steps; x starts at zero (uninitialised in the
    // reference) and keeps its value through qr_solve's early return
    for (int k = 0; k < 4; k++) W.x[k] = 0.0;
    for (int step = 0; step < 5; step++) {
        for (int i = 0; i < 6; i++) {
            const double* r = S.L + 10 * i;
            W.A[4 * i] = ((2 * r[0] * be[0] + r[1] * be[1]) + r[3] * be[2]) + r[6] * be[3];
            W.A[4 * i + 1] = ((r[1] * be[0] + 2 * r[2] * be[1]) + r[4] * be[2]) + r[7] * be[3];
            W.A[4 * i + 2] = ((r[3] * be[0] + r[4] * be[1]) + 2 * r[5] * be[2]) + r[8] * be[3];
            W.A[4 * i + 3] = ((r[6] * be[0] + r[7] * be[1]) + r[8] * be[2]) + 2 * r[9] * be[3];
            double s = r[0] * be[0] * be[0] + r[1] * be[0] * be[1];
            s = s + r[2] * be[1] * be[1];
            s = s + r[3] * be[0] * be[2];
            s = s + r[4] * be[1] * be[2];
            s = s + r[5] * be[2] * be[2];
            s = s + r[6] * be[0] * be[3];
            s = s + r[7] * be[1] * be[3];
            s = s + r[8] * be[2] * be[3];
            s = s + r[9] * be[3] * be[3];
            W.b[i] = S.rho[i] - s;
        }
        // qr_solve (:832-922), nr = 6, nc = 4
        bool singular = false;
        for (int k = 0; k < 4 && !singular; k++) {
            const int kk = 5 * k;
            double eta = fabs(W.A[kk]);
            for (int i = k + 1; i < 6; i++) {   // the reference's walk starts at row k again
                const double elt = fabs(W.A[kk + (i - k - 1) * 4]);
                if (eta < elt) eta = elt;
            }
            if (eta == 0) {
                singular = true;
                break;
            }
            const double inv_eta = 1. / eta;
            double sum = 0.0;
            for (int i = k; i < 6; i++) {
                W.A[i * 4 + k] *= inv_eta;
                sum += W.A[i * 4 + k] * W.A[i * 4 + k];
            }
            double sigma = sqrt(sum);
            if (W.A[kk] < 0) sigma = -sigma;
            W.A[kk] += sigma;
            W.A1[k] = sigma * W.A[kk];
            W.A2[k] = -eta * sigma;
            for (int j = k + 1; j < 4; j++) {
                double s2 = 0;
                for (int i = k; i < 6; i++) s2 += W.A[i * 4 + k] * W.A[i * 4 + j];
                const double tau = s2 / W.A1[k];
                for (int i = k; i < 6; i++) W.A[i * 4 + j] -= tau * W.A[i * 4 + k];
            }
        }
        if (!singular) {
            for (int j = 0; j < 4; j++) {
                double tau = 0;
                for (int i = j; i < 6; i++) tau += W.A[i * 4 + j] * W.b[i];
                tau /= W.A1[j];
                for (int i = j; i < 6; i++) W.b[i] -= tau * W.A[i * 4 + j];
            }
            W.x[3] = W.b[3] / W.A2[3];
            for (int i = 2; i >= 0; i--) {
                double s2 = 0;
                for (int j = i + 1; j < 4; j++) s2 += W.A[i * 4 + j] * W.x[j];
                W.x[i] = (W.b[i] - s2) / W.A2[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) be[i] += W.x[i];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) rec[R_BETAS + 4 * (which - 1) + i] = be[i];
    // compute_ccs (:425-436): v[i] is row 11 - i of Ut
    double ccs[12];
#pragma unroll
    for (int k = 0; k < 12; k++) ccs[k] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 12; k++) ccs[k] += be[i] * S.ut[12 * (3 - i) + k];
    // compute_pcs of a point (:438-447)
    auto pc_of = [&](int i, double* pc) {
        double a[4];
        epnp_alphas(P, i, S.cws, S.ci, a);
#pragma unroll
        for (int j = 0; j < 3; j++) pc[j] = ((a[0] * ccs[j] + a[1] * ccs[3 + j]) + a[2] * ccs[6 + j]) + a[3] * ccs[9 + j];
    };
    // solve_for_sign (:608-621)
    double pc[3];
    pc_of(0, pc);
    const double sign = pc[2] < 0.0 ? -1.0 : 1.0;
    // estimate_R_and_t (:541-599)
    double pc0[3] = {0.0, 0.0, 0.0}, pw0[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < n; i++) {
        pc_of(i, pc);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            pc0[j] += sign * pc[j];
            pw0[j] += P.pw(i, j);
        }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        pc0[j] /= n;
        pw0[j] /= n;
    }
    double abt[9];
#pragma unroll
    for (int k = 0; k < 9; k++) abt[k] = 0.0;
    for (int i = 0; i < n; i++) {
        pc_of(i, pc);
        const double w0 = P.pw(i, 0) - pw0[0], w1 = P.pw(i, 1) - pw0[1], w2 = P.pw(i, 2) - pw0[2];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double c = sign * pc[j] - pc0[j];
            abt[3 * j] += c * w0;
            abt[3 * j + 1] += c * w1;
            abt[3 * j + 2] += c * w2;
        }
    }
    // (e) cvSVD of ABt: U and V as matrices, a vanishing third direction
    // completed by the cross product of the other two
    for (int k = 0; k < 9; k++) W.abt[k] = abt[k];
    svd_cols(W.abt, 3, 3, W.av);
    {
        double w[3], wsum = 0.0;
        for (int j = 0; j < 3; j++) {
            w[j] = sqrt((W.abt[j] * W.abt[j] + W.abt[3 + j] * W.abt[3 + j]) + W.abt[6 + j] * W.abt[6 + j]);
            wsum += w[j];
        }
        const double cut = 2.0 * DBL_EPSILON * wsum;
        int small = 0, which_small = -1;
        for (int j = 0; j < 3; j++)
            if (!(w[j] > cut)) {
                small++;
                which_small = j;
            }
        for (int j = 0; j < 3; j++) {
            const double wi = sv_inv(w[j], cut);
            for (int i = 0; i < 3; i++) W.abt[3 * i + j] *= wi;
        }
        if (small == 1) {
            const int a = (which_small + 1) % 3, c = (which_small + 2) % 3;
            W.abt[which_small] = W.abt[3 + a] * W.abt[6 + c] - W.abt[6 + a] * W.abt[3 + c];
            W.abt[3 + which_small] = W.abt[6 + a] * W.abt[c] - W.abt[a] * W.abt[6 + c];
            W.abt[6 + which_small] = W.abt[a] * W.abt[3 + c] - W.abt[3 + a] * W.abt[c];
        }
    }
    double U[9], V[9];   // matrices: V[3*j + k] is component j of right vector k
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            U[3 * i + j] = W.abt[3 * i + j];
            V[3 * i + j] = W.av[3 * j + i];
        }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        rec[R_UV + 18 * (which - 1) + k] = U[k];
        rec[R_UV + 18 * (which - 1) + 9 + k] = V[k];
    }
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            R[3 * i + j] = (U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1]) + U[3 * i + 2] * V[3 * j + 2];
    double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6];
    det = det + R[2] * R[3] * R[7];
    det = det - R[2] * R[4] * R[6];
    det = det - R[1] * R[3] * R[8];
    det = det - R[0] * R[5] * R[7];
    if (det < 0) {
        R[6] = -R[6];
        R[7] = -R[7];
        R[8] = -R[8];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = pc0[i] - ((R[3 * i] * pw0[0] + R[3 * i + 1] * pw0[1]) + R[3 * i + 2] * pw0[2]);
    // reprojection_error (:522-539)
    const double fu = camd[0], fv = camd[1], uc = camd[2], vc = camd[3];
    double sum2 = 0.0;
    for (int i = 0; i < n; i++) {
        const double x = P.pw(i, 0), y = P.pw(i, 1), z = P.pw(i, 2);
        const double Xc = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
        const double Yc = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
        const double inv_Zc = 1.0 / (((R[6] * x + R[7] * y) + R[8] * z) + t[2]);
        const double ue = uc + fu * Xc * inv_Zc;
        const double ve = vc + fv * Yc * inv_Zc;
        const double u = P.u(i, 0), v = P.u(i, 1);
        sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
    }
#pragma unroll
    for (int k = 0; k < 9; k++) W.R[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) W.t[k] = t[k];
    W.err = sum2 / n;
}

// compute_pose (:449-497) of one hypothesis by the kPnpLanes lanes of a
// group (gl the lane's index in it); every wave-level barrier is reached by
// all lanes of the workgroup, whatever `act` is.  rec: the hypothesis record.
__device__ inline void epnp(const EpnpPoints& P, bool act, int gl, EpnpLds& S, const float* cam, double* rec)
{
    const int n = P.n;
    act = act && n > 0;
    const double camd[4] = {(double)cam[0], (double)cam[1], (double)cam[2], (double)cam[3]};
    if (act && gl == 0) {
        // choose_control_points (:347-381)
        double c0[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < n; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) c0[j] += P.pw(i, j);
#pragma unroll
        for (int j = 0; j < 3; j++) c0[j] /= n;
        // (a) cvMulTransposed: the rows in their order
        double g[9];
#pragma unroll
        for (int k = 0; k < 9; k++) g[k] = 0.0;
        for (int i = 0; i < n; i++) {
            const double d[3] = {P.pw(i, 0) - c0[0], P.pw(i, 1) - c0[1], P.pw(i, 2) - c0[2]};
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) g[3 * r + c] += d[r] * d[c];
        }
        for (int k = 0; k < 9; k++) S.g3[k] = g[k];
        // (b) cvSVD of the symmetric matrix: eigenvectors as rows, |eigenvalue| descending
        sym_eig<false>(S.g3, S.v3, 3, 0, 1, true);
        double dc[3], uct[9];
        for (int j = 0; j < 3; j++) {
            const double lam = fabs(S.g3[4 * j]);
            int rank = 0;
            for (int i = 0; i < 3; i++) {
                const double li = fabs(S.g3[4 * i]);
                rank += (li > lam) || (li == lam && i < j);
            }
#pragma unroll
            for (int r = 0; r < 3; r++)
                if (rank == r) {
                    dc[r] = lam;
                    uct[3 * r] = S.v3[3 * j];
                    uct[3 * r + 1] = S.v3[3 * j + 1];
                    uct[3 * r + 2] = S.v3[3 * j + 2];
                }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) rec[R_DC + k] = dc[k];
#pragma unroll
        for (int k = 0; k < 9; k++) rec[R_UCT + k] = uct[k];
        double cws[12];
#pragma unroll
        for (int j = 0; j < 3; j++) cws[j] = c0[j];
#pragma unroll
        for (int i = 1; i < 4; i++) {
            const double k = sqrt(dc[i - 1] / n);
#pragma unroll
            for (int j = 0; j < 3; j++) cws[3 * i + j] = c0[j] + k * uct[3 * (i - 1) + j];
        }
        for (int k = 0; k < 12; k++) S.cws[k] = cws[k];
        // compute_barycentric_coordinates (:383-393); (c) cvInvert(CV_SVD)
        for (int i = 0; i < 3; i++)
            for (int j = 1; j < 4; j++) S.cc[3 * i + j - 1] = cws[3 * j + i] - cws[i];
        svd_cols(S.cc, 3, 3, S.vc);
        {
            double w[3], wsum = 0.0;
            for (int j = 0; j < 3; j++) {
                w[j] = sqrt((S.cc[j] * S.cc[j] + S.cc[3 + j] * S.cc[3 + j]) + S.cc[6 + j] * S.cc[6 + j]);
                wsum += w[j];
            }
            const double cut = 2.0 * DBL_EPSILON * wsum;
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) {
                    double s = 0.0;
                    for (int j = 0; j < 3; j++) {
                        const double wi = sv_inv(w[j], cut);
                        s += (S.vc[3 * j + r] * wi) * (S.cc[3 * c + j] * wi);
                    }
                    S.ci[3 * r + c] = s;
                    rec[R_CI + 3 * r + c] = s;
                }
        }
        // compute_rho (:774-782)
        const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const double* a = cws + 3 * pa[k];
            const double* b = cws + 3 * pb[k];
            const double r = ((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1])) + (a[2] - b[2]) * (a[2] - b[2]);
            S.rho[k] = r;
            rec[R_RHO + k] = r;
        }
    }
    __syncthreads();
    // fill_M (:408-423) and (a) MtM: the 78 entries of the upper triangle over
    // the lanes, the 2n rows in their order, the zero entries multiplied too
    if (act) {
        int er[5], ec[5];
        {
            int r = 0, c = 0;
#pragma unroll
            for (int k = 0; k < 5; k++) er[k] = ec[k] = -1;
            for (int cnt = 0; cnt < 78; cnt++) {
                if (cnt % kPnpLanes == gl) {
                    const int k = cnt / kPnpLanes;
#pragma unroll
                    for (int q = 0; q < 5; q++)
                        if (q == k) {
                            er[q] = r;
                            ec[q] = c;
                        }
                }
                c++;
                if (c == 12) {
                    r++;
                    c = r;
                }
            }
        }
        double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        const double f0 = camd[0], f1 = camd[1];
        for (int i = 0; i < n; i++) {
            double a[4];
            epnp_alphas(P, i, S.cws, S.ci, a);
            const double du = camd[2] - P.u(i, 0), dv = camd[3] - P.u(i, 1);
#pragma unroll
            for (int q = 0; q < 5; q++)
                if (er[q] >= 0) {
                    acc[q] += epnp_m(a, 0, er[q], f0, f1, du, dv) * epnp_m(a, 0, ec[q], f0, f1, du, dv);
                    acc[q] += epnp_m(a, 1, er[q], f0, f1, du, dv) * epnp_m(a, 1, ec[q], f0, f1, du, dv);
                }
        }
#pragma unroll
        for (int q = 0; q < 5; q++)
            if (er[q] >= 0) {
                S.A[er[q] * 12 + ec[q]] = acc[q];
                S.A[ec[q] * 12 + er[q]] = acc[q];
            }
        for (int k = gl; k < 48; k += kPnpLanes) S.ut[k] = __builtin_nan("");
    }
    __syncthreads();
    // (b) cvSVD of MtM: rows 8..11 of Ut
    sym_eig<true>(S.A, S.V, 12, gl, kPnpLanes, act);
    if (act && gl < 12) {
        const double lam = fabs(S.A[13 * gl]);
        int rank = 0;
        for (int i = 0; i < 12; i++) {
            const double li = fabs(S.A[13 * i]);
            rank += (li > lam) || (li == lam && i < gl);
        }
        if (rank >= 8 && lam == lam)
            for (int k = 0; k < 12; k++) S.ut[12 * (rank - 8) + k] = S.V[12 * gl + k];
    }
    __syncthreads();
    if (act) {
        for (int k = gl; k < 48; k += kPnpLanes) rec[R_UT + k] = S.ut[k];
        // compute_L_6x10 (:732-772): a lane per row
        if (gl < 6) {
            const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
            int a = 0, b = 1;
#pragma unroll
            for (int k = 0; k < 6; k++)
                if (k == gl) {
                    a = pa[k];
                    b = pb[k];
                }
            double dv[4][3];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const double* v = S.ut + 12 * (3 - i);
#pragma unroll
                for (int k = 0; k < 3; k++) dv[i][k] = v[3 * a + k] - v[3 * b + k];
            }
            auto dot = [](const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; };
            double row[10];
            row[0] = dot(dv[0], dv[0]);
            row[1] = 2.0 * dot(dv[0], dv[1]);
            row[2] = dot(dv[1], dv[1]);
            row[3] = 2.0 * dot(dv[0], dv[2]);
            row[4] = 2.0 * dot(dv[1], dv[2]);
            row[5] = dot(dv[2], dv[2]);
            row[6] = 2.0 * dot(dv[0], dv[3]);
            row[7] = 2.0 * dot(dv[1], dv[3]);
            row[8] = 2.0 * dot(dv[2], dv[3]);
            row[9] = dot(dv[3], dv[3]);
#pragma unroll
            for (int k = 0; k < 10; k++) {
                S.L[10 * gl + k] = row[k];
                rec[R_L + 10 * gl + k] = row[k];
            }
        }
    }
    __syncthreads();
    // the three beta sets, a lane each
    if (act && gl < 3) epnp_branch(gl + 1, P, S, S.br[gl], camd, rec);
    __syncthreads();
    if (act && gl == 0) {
        int pick = 1;
        if (S.br[1].err < S.br[0].err) pick = 2;
        if (S.br[2].err < S.br[pick - 1].err) pick = 3;
        const EpnpBranch& W = S.br[pick - 1];
        for (int k = 0; k < 9; k++) rec[R_R + k] = W.R[k];
        for (int k = 0; k < 3; k++) rec[R_T + k] = W.t[k];
        for (int k = 0; k < 3; k++) rec[R_ERR + k] = S.br[k].err;
        rec[R_CHOSEN] = (double)pick;
    }
    __syncthreads();
}

// A record no hypothesis wrote: NaNs, the chosen set 0 (the buffer was cleared).
__device__ inline void rec_init(double* rec, int gl, int npts)
{
    for (int k = gl; k < kRec; k += kPnpLanes) rec[k] = (k == R_CHOSEN || k >= R_NPTS) ? 0.0 : __builtin_nan("");
    if (gl == 0) rec[R_NPTS] = (double)npts;
}

__global__ __launch_bounds__(64) void k_pnp_solve(const PnpCand* __restrict__ cands, uint8_t* __restrict__ res,
                                                  PnpLayout L)
{
    __shared__ EpnpLds s_lds[kPnpGroups];
    const PnpCand& d = cands[blockIdx.y];
    uint8_t* blk = res + (long long)blockIdx.y * L.stride;
    const PnpHdr* hdr = reinterpret_cast<const PnpHdr*>(blk);
    const int E = min(hdr->E, L.M);
    if (blockIdx.x * kPnpGroups >= E) return;   // uniform
    const int group = threadIdx.x / kPnpLanes, gl = threadIdx.x % kPnpLanes;
    const int it = blockIdx.x * kPnpGroups + group;
    const bool act = it < E;
    const int N = hdr->N;
    const int32_t* set = reinterpret_cast<const int32_t*>(blk + L.o_sets) + (act ? it : 0) * 4;
    // the set's indices, clamped
    __shared__ int32_t s_idx[kPnpGroups][4];
    if (gl < 4) s_idx[group][gl] = act ? min(max(set[gl], 0), max(N - 1, 0)) : 0;
    __syncthreads();
    EpnpPoints P;
    P.idx = s_idx[group];
    P.p3 = reinterpret_cast<const float*>(blk + L.o_p3);
    P.p2 = reinterpret_cast<const float*>(blk + L.o_p2);
    P.n = 4;
    double* rec = reinterpret_cast<double*>(blk + L.o_rec) + (long long)(act ? it : 0) * kRec;
    if (act) rec_init(rec, gl, 4);
    __syncthreads();
    epnp(P, act, gl, s_lds[group], d.cam, rec);
}

// ---------------------------------------------------------------------------
// CheckInliers (:280-311)
// ---------------------------------------------------------------------------
// Of one correspondence c (p3d 0..2, p2d 3..4, mvMaxError 5) under R (9) and
// t (3): the mixed float / double expressions as C++ evaluates them.  Under
// contract the sums of products fuse left to right.  NaNs fail the test.
__device__ inline bool pnp_inlier(const float* c, const double* R, const double* t, const double* camd, int contract)
{
    const double x = (double)c[0], y = (double)c[1], z = (double)c[2];
    double r[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
        r[i] = contract ? fma(R[3 * i + 2], z, fma(R[3 * i + 1], y, R[3 * i] * x)) + t[i]
                        : ((R[3 * i] * x + R[3 * i + 1] * y) + R[3 * i + 2] * z) + t[i];
    const float Xc = (float)r[0], Yc = (float)r[1];
    const float invZc = (float)(1.0 / r[2]);
    const double fu = camd[0], fv = camd[1], uc = camd[2], vc = camd[3];
    const double ue = contract ? fma(fu * (double)Xc, (double)invZc, uc) : uc + fu * (double)Xc * (double)invZc;
    const double ve = contract ? fma(fv * (double)Yc, (double)invZc, vc) : vc + fv * (double)Yc * (double)invZc;
    const float distX = (float)((double)c[3] - ue);
    const float distY = (float)((double)c[4] - ve);
    const float error2 = contract ? fmaf(distX, distX, distY * distY) : distX * distX + distY * distY;
    return error2 < c[5];
}

__device__ inline void pnp_corr(const uint8_t* blk, const PnpLayout& L, int g, float* c)
{
    const float* p3 = reinterpret_cast<const float*>(blk + L.o_p3);
    const float* p2 = reinterpret_cast<const float*>(blk + L.o_p2);
    c[0] = p3[3 * g];
    c[1] = p3[3 * g + 1];
    c[2] = p3[3 * g + 2];
    c[3] = p2[2 * g];
    c[4] = p2[2 * g + 1];
    c[5] = reinterpret_cast<const float*>(blk + L.o_me)[g];
}

__device__ inline void pnp_pose(const double* rec, double* R, double* t)
{
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = rec[R_R + k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = rec[R_T + k];
}

__global__ __launch_bounds__(1024) void k_pnp_check(const PnpCand* __restrict__ cands, uint8_t* __restrict__ res,
                                                    PnpLayout L, int contract)
{
    __shared__ float s_c[kPnpTile * kPnpFloats];
    __shared__ int s_count[kPnpMaxIter];
    const PnpCand& d = cands[blockIdx.x];
    uint8_t* blk = res + (long long)blockIdx.x * L.stride;
    PnpHdr* hdr = reinterpret_cast<PnpHdr*>(blk);
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int E = min(min(hdr->E, L.M), kPnpMaxIter);
    const int N = min(hdr->N, L.cap);
    if (!hdr->run || E <= 0) {   // uniform
        if (tid == 0) hdr->n_rec = 0;
        return;
    }
    const double camd[4] = {(double)d.cam[0], (double)d.cam[1], (double)d.cam[2], (double)d.cam[3]};
    const double* recs = reinterpret_cast<const double*>(blk + L.o_rec);
    int32_t* count = reinterpret_cast<int32_t*>(blk + L.o_cnt);
    for (int i = tid; i < E; i += nthreads) s_count[i] = 0;
    // a lane per (iteration, slice): the lanes of a wave share the
    // correspondence (LDS broadcast) and differ in the iteration
    const int S = max(1, nthreads / E);
    for (int first = 0; first < N; first += kPnpTile) {
        const int cnt = min(kPnpTile, N - first);
        __syncthreads();
        for (int i = tid; i < cnt; i += nthreads) pnp_corr(blk, L, first + i, s_c + i * kPnpFloats);
        __syncthreads();
        for (int w = tid; w < E * S; w += nthreads) {
            const int it = w % E, slice = w / E;
            double R[9], t[3];
            pnp_pose(recs + (long long)it * kRec, R, t);
            int c = 0;
            for (int i = slice; i < cnt; i += S) c += pnp_inlier(s_c + i * kPnpFloats, R, t, camd, contract);
            if (c) atomicAdd(&s_count[it], c);
        }
    }
    __syncthreads();
    for (int i = tid; i < E; i += nthreads) count[i] = s_count[i];
    // the strict record holders among the iterations with count >= min (:181-196)
    if (tid == 0) {
        int32_t* recl = reinterpret_cast<int32_t*>(blk + L.o_recl);
        int best = d.best_in, n_rec = 0;
        recl[0] = -1;
        for (int it = 0; it < E; it++) {
            const int c = s_count[it];
            if (c >= hdr->min_inl && c > best && n_rec + 1 < L.K) {
                best = c;
                recl[++n_rec] = it;
            }
        }
        hdr->n_rec = n_rec;
    }
}

// ---------------------------------------------------------------------------
// k_pnp_refine, k_pnp_select
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pnp_refine(const PnpCand* __restrict__ cands, uint8_t* __restrict__ res,
                                                   PnpLayout L, int contract)
{
    __shared__ EpnpLds s_lds;
    const PnpCand& d = cands[blockIdx.y];
    uint8_t* blk = res + (long long)blockIdx.y * L.stride;
    const PnpHdr* hdr = reinterpret_cast<const PnpHdr*>(blk);
    if (!hdr->run) return;   // uniform
    const int lane = threadIdx.x;
    const int N = min(hdr->N, L.cap);
    const int n_rec = min(hdr->n_rec, L.K - 1);
    const double camd[4] = {(double)d.cam[0], (double)d.cam[1], (double)d.cam[2], (double)d.cam[3]};
    const int32_t* kp = reinterpret_cast<const int32_t*>(blk + L.o_kp);
    const int32_t* recl = reinterpret_cast<const int32_t*>(blk + L.o_recl);
    const double* recs = reinterpret_cast<const double*>(blk + L.o_rec);
    double* rrecs = reinterpret_cast<double*>(blk + L.o_rrec);
    int32_t* rcnt = reinterpret_cast<int32_t*>(blk + L.o_rcnt);
    int32_t* ridx = reinterpret_cast<int32_t*>(blk + L.o_ridx) + (long long)blockIdx.x * L.cap;
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int s = blockIdx.x; s <= n_rec; s += gridDim.x) {   // uniform
        if (s == 0 && d.best_in <= 0) continue;   // a fresh solver has no set to refit
        // mvbBestInliers of the slot, compacted in order (:237-243)
        double R[9], t[3];
        if (s > 0) pnp_pose(recs + (long long)recl[s] * kRec, R, t);
        int base = 0;
        for (int c0 = 0; c0 < N; c0 += 64) {
            const int g = c0 + lane;
            bool in = false;
            if (g < N) {
                if (s == 0) {
                    in = d.mask_in[kp[g]] != 0;
                } else {
                    float c[kPnpFloats];
                    pnp_corr(blk, L, g, c);
                    in = pnp_inlier(c, R, t, camd, contract);
                }
            }
            const unsigned long long bal = __ballot(in);
            if (in) ridx[base + __popcll(bal & lt_mask)] = g;
            base += __popcll(bal);
        }
        __syncthreads();
        EpnpPoints P;
        P.idx = ridx;
        P.p3 = reinterpret_cast<const float*>(blk + L.o_p3);
        P.p2 = reinterpret_cast<const float*>(blk + L.o_p2);
        P.n = base;
        double* rec = rrecs + (long long)s * kRec;
        if (lane < kPnpLanes) rec_init(rec, lane, base);
        __syncthreads();
        epnp(P, lane < kPnpLanes, lane % kPnpLanes, s_lds, d.cam, rec);
        // CheckInliers of the refit (:259-262)
        pnp_pose(rec, R, t);
        int cnt = 0;
        for (int c0 = 0; c0 < N; c0 += 64) {
            const int g = c0 + lane;
            bool in = false;
            if (g < N) {
                float c[kPnpFloats];
                pnp_corr(blk, L, g, c);
                in = pnp_inlier(c, R, t, camd, contract);
            }
            cnt += __popcll(__ballot(in));
        }
        if (lane == 0) rcnt[s] = cnt;
        __syncthreads();
    }
}

__device__ inline void tcw_of(const double* rec, float* T)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) T[4 * i + j] = (float)rec[R_R + 3 * i + j];
        T[4 * i + 3] = (float)rec[R_T + i];
        T[12 + i] = 0.f;
    }
    T[15] = 1.f;
}

__global__ __launch_bounds__(256) void k_pnp_select(const PnpCand* __restrict__ cands, uint8_t* __restrict__ res,
                                                    PnpLayout L, int contract)
{
    __shared__ int s_ret, s_slot;   // the refit slot whose mask is returned (-1: the best set's, -2: none)
    const PnpCand& d = cands[blockIdx.x];
    uint8_t* blk = res + (long long)blockIdx.x * L.stride;
    PnpHdr* hdr = reinterpret_cast<PnpHdr*>(blk);
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int n = max(0, min(d.n, L.cap));
    const int N = min(hdr->N, L.cap);
    const int32_t* count = reinterpret_cast<const int32_t*>(blk + L.o_cnt);
    const int32_t* recl = reinterpret_cast<const int32_t*>(blk + L.o_recl);
    const int32_t* rcnt = reinterpret_cast<const int32_t*>(blk + L.o_rcnt);
    const double* recs = reinterpret_cast<const double*>(blk + L.o_rec);
    const double* rrecs = reinterpret_cast<const double*>(blk + L.o_rrec);
    if (tid == 0) {
        const int E = hdr->run ? min(min(hdr->E, L.M), kPnpMaxIter) : 0;
        const int min_inl = hdr->min_inl;
        int best = d.best_in, slot = 0, found = -1;
        // iterate's loop (:154-211) over the counts
        for (int it = 0; it < E; it++) {
            const int c = count[it];
            if (c >= min_inl) {
                if (c > best && slot < hdr->n_rec) {
                    best = c;
                    slot++;
                }
                if (rcnt[slot] > min_inl) {   // Refine (:264), strict
                    found = it;
                    break;
                }
            }
        }
        int ret = -2;
        hdr->iters_run = found >= 0 ? found + 1 : E;
        hdr->iter_out = d.iter_done + hdr->iters_run;
        hdr->found_iter = found;
        hdr->best_out = best;
        hdr->best_slot = slot;
        if (slot > 0)
            tcw_of(recs + (long long)recl[slot] * kRec, hdr->best_Tcw);
        else
            for (int k = 0; k < 16; k++) hdr->best_Tcw[k] = d.Tcw_in[k];
        hdr->found = 0;
        hdr->refined = 0;
        hdr->n_inliers = 0;
        hdr->no_more = 0;
        if (found >= 0) {
            hdr->found = 1;
            hdr->refined = 1;
            hdr->n_inliers = rcnt[slot];
            tcw_of(rrecs + (long long)slot * kRec, hdr->Tcw);
            ret = slot;
        } else if (!hdr->discarded) {
            // (:145-149) or the loop ran out: mnIterations >= mRansacMaxIts holds (:213)
            hdr->no_more = 1;
            if (hdr->run && best >= min_inl) {
                hdr->found = 1;
                hdr->n_inliers = best;
                for (int k = 0; k < 16; k++) hdr->Tcw[k] = hdr->best_Tcw[k];
                ret = -1;
            }
        }
        s_ret = ret;
        s_slot = slot;
    }
    __syncthreads();
    const int ret = s_ret, slot = s_slot;
    uint8_t* inl = blk + L.o_inl;
    uint8_t* mask = blk + L.o_mask;
    const int32_t* kp = reinterpret_cast<const int32_t*>(blk + L.o_kp);
    const double camd[4] = {(double)d.cam[0], (double)d.cam[1], (double)d.cam[2], (double)d.cam[3]};
    // mvbBestInliers at return: the incoming mask, or the last record holder's, recomputed
    if (slot == 0) {
        for (int i = tid; i < n; i += nthreads) {
            const uint8_t m = d.mask_in[i] ? 1 : 0;
            mask[i] = m;
            if (ret == -1) inl[i] = m;
        }
    } else {
        double R[9], t[3];
        pnp_pose(recs + (long long)recl[slot] * kRec, R, t);
        for (int g = tid; g < N; g += nthreads) {
            float c[kPnpFloats];
            pnp_corr(blk, L, g, c);
            if (pnp_inlier(c, R, t, camd, contract)) {
                mask[kp[g]] = 1;
                if (ret == -1) inl[kp[g]] = 1;
            }
        }
    }
    if (ret >= 0) {   // mvbRefinedInliers (:262)
        double R[9], t[3];
        pnp_pose(rrecs + (long long)ret * kRec, R, t);
        for (int g = tid; g < N; g += nthreads) {
            float c[kPnpFloats];
            pnp_corr(blk, L, g, c);
            if (pnp_inlier(c, R, t, camd, contract)) inl[kp[g]] = 1;
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {

int launch_pnp(orbx_ctx* ctx, int P, const PnpCand* cands, uint8_t* res, const PnpLayout& L)
{
    hipStream_t st = ctx->stream;
    const int contract = ctx->fp_contract;
    timer_begin(ctx, "pnp");
    timer_begin(ctx, "pnp.prepare");
    hipLaunchKernelGGL(k_pnp_prepare, dim3(P), dim3(256), 0, st, cands, res, L);
    timer_end(ctx, "pnp.prepare");
    ORBX_HIP_CHECK(hipGetLastError());
    timer_begin(ctx, "pnp.solve");
    hipLaunchKernelGGL(k_pnp_solve, dim3((L.M + kPnpGroups - 1) / kPnpGroups, P), dim3(64), 0, st, cands, res, L);
    timer_end(ctx, "pnp.solve");
    ORBX_HIP_CHECK(hipGetLastError());
    timer_begin(ctx, "pnp.check");
    hipLaunchKernelGGL(k_pnp_check, dim3(P), dim3(1024), 0, st, cands, res, L, contract);
    timer_end(ctx, "pnp.check");
    ORBX_HIP_CHECK(hipGetLastError());
    timer_begin(ctx, "pnp.refine");
    hipLaunchKernelGGL(k_pnp_refine, dim3(kPnpRefineBlocks, P), dim3(64), 0, st, cands, res, L, contract);
    hipLaunchKernelGGL(k_pnp_select, dim3(P), dim3(256), 0, st, cands, res, L, contract);
    timer_end(ctx, "pnp.refine");
    timer_end(ctx, "pnp");
    ORBX_HIP_CHECK(hipGetLastError());
    return ORBX_OK;
}

// SetRansacParameters (:93-124) for N correspondences: the float product
// truncated, the float epsilon, the double log / pow / ceil.  max_its is
// reported as 0 when N < min_inliers (no iteration runs there).
void ransac_parameters(int N, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                       int* out_min, int* out_its)
{
    int nMinInliers = (int)((float)N * epsilon);
    if (nMinInliers < min_inliers) nMinInliers = min_inliers;
    if (nMinInliers < min_set) nMinInliers = min_set;
    *out_min = nMinInliers;
    *out_its = 0;
    if (N < nMinInliers) return;
    float eps = epsilon;
    if (eps < (float)nMinInliers / N) eps = (float)nMinInliers / N;
    const int nIterations = nMinInliers == N ? 1 : ransac_iterations(eps, probability);
    *out_its = std::max(1, std::min(nIterations, max_iterations));
}

// The rules shared by the host forms and the slot form.
int check_params(const orbx_pnp_query& q)
{
    if (q.min_set != 4) return ORBX_ERR_UNSUPPORTED;
    if (q.n_iter < 1 || !q.draws || q.min_inliers < 1 || q.max_iterations < 1 ||
        !(q.probability > 0.0 && q.probability < 1.0) || !(q.epsilon >= 0.f && q.epsilon <= 1.f) ||
        !(q.th2 > 0.f && q.th2 <= FLT_MAX) || q.iter_done < 0 || q.best_inliers < 0 || !q.inliers || !q.best_mask)
        return ORBX_ERR_ARG;
    const long long need = std::max((long long)q.n_iter, (long long)q.max_iterations - q.iter_done);
    if (q.n_draws < need || q.n_draws > kPnpMaxIter) return ORBX_ERR_ARG;
    for (long long i = 0; i < (long long)q.n_draws * 4; i++)
        if (q.draws[i] < 0) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// Finite and not negative: nothing here converts a multiple of it to int, as
// orbx_sim3.hip's kernels do.
bool sigma2_ok(const float* s, int nlevels)
{
    if (!s) return false;
    for (int l = 0; l < nlevels; l++)
        if (!(s[l] >= 0.f && s[l] <= FLT_MAX)) return false;
    return true;
}

// One candidate's result block (host copy) into the query's outputs and taps.
void scatter(const uint8_t* blk, const PnpLayout& L, int n, orbx_pnp_query* q)
{
    const PnpHdr* h = reinterpret_cast<const PnpHdr*>(blk);
    q->N = h->N;
    q->ransac_min_inliers = h->min_inl;
    q->ransac_max_its = h->max_its;
    q->iters_run = h->iters_run;
    q->no_more = h->no_more;
    q->found = h->found;
    q->found_iter = h->found_iter;
    q->n_inliers = h->n_inliers;
    q->refined = h->refined;
    q->n_records = h->n_rec;
    q->best_slot = h->best_slot;
    if (h->found) std::memcpy(q->Tcw, h->Tcw, sizeof(q->Tcw));
    q->iter_done = h->iter_out;
    q->best_inliers = h->best_out;
    std::memcpy(q->best_Tcw, h->best_Tcw, sizeof(q->best_Tcw));
    const int m = std::max(0, std::min(n, std::min(q->cap, L.cap)));
    if (m > 0) {
        std::memcpy(q->inliers, blk + L.o_inl, m);
        std::memcpy(q->best_mask, blk + L.o_mask, m);
    }
    auto tap = [&](void* dst, long long off, size_t bytes) {
        if (dst && bytes) std::memcpy(dst, blk + off, bytes);
    };
    const size_t M = (size_t)std::max(0, std::min(q->n_draws, L.M));
    const size_t K = std::min(M + 1, (size_t)L.K);
    tap(q->sets, L.o_sets, M * 16);
    tap(q->rec, L.o_rec, M * kRec * 8);
    tap(q->count, L.o_cnt, M * 4);
    tap(q->refit_rec, L.o_rrec, K * kRec * 8);
    tap(q->refit_count, L.o_rcnt, K * 4);
    tap(q->record_iter, L.o_recl, K * 4);
    const size_t N = (size_t)std::max(0, std::min(h->N, m));
    tap(q->p2d, L.o_p2, N * 8);
    tap(q->p3d, L.o_p3, N * 12);
    tap(q->max_err, L.o_me, N * 4);
    tap(q->kp_index, L.o_kp, N * 4);
}

bool wants_taps(const orbx_pnp_query& q)
{
    return q.p2d || q.p3d || q.max_err || q.kp_index || q.sets || q.rec || q.count || q.refit_rec || q.refit_count ||
           q.record_iter;
}

// What is read back of a result block: all of it when a tap is asked for,
// else its head (header and the two masks).
size_t read_bytes(const PnpLayout& L, int n, const orbx_pnp_query* qs)
{
    return std::any_of(qs, qs + n, wants_taps) ? (size_t)L.stride : (size_t)L.head;
}

}  // namespace
}  // namespace orbx

using namespace orbx;

extern "C" int orbx_pnp_ransac_batch(orbx_ctx* ctx, int B, orbx_pnp_query* qs)
{
    if (!ctx || !qs || B < 1) return ORBX_ERR_ARG;
    // argument rules, before any device work; what travels is taken as it is checked:
    // descriptors | per candidate: keypoints, positions, sigma2, flags, mask, draws
    struct Staged {
        Region<orbx_keypoint> keys;
        Region<float> pos, sigma2;
        Region<uint8_t> valid, mask;
        Region<int32_t> draws;
    };
    int Mmax = 1, cap = 1;
    std::vector<int> Ns(B);
    std::vector<Staged> at(B);
    PackedStage st(ctx);
    const Region<PnpCand> cands = st.take<PnpCand>(B);
    for (int b = 0; b < B; b++) {
        const orbx_pnp_query& q = qs[b];
        if (q.n < 0 || (q.n > 0 && (!q.keys || !q.pos || !q.valid)) || !q.cam) return ORBX_ERR_ARG;
        int r = check_params(q);
        if (r != ORBX_OK) return r;
        if (q.nlevels < 1 || q.nlevels > kMaxLevels || !sigma2_ok(q.sigma2, q.nlevels)) return ORBX_ERR_ARG;
        if (q.n > kMaxFeatures) return ORBX_ERR_UNSUPPORTED;
        if (!octaves_ok(q.keys, q.n, q.nlevels)) return ORBX_ERR_ARG;
        int N = 0;
        for (int i = 0; i < q.n; i++) N += q.valid[i] != 0;
        if (q.cap < q.n) return ORBX_ERR_CAPACITY;
        Ns[b] = N;
        Mmax = std::max(Mmax, q.n_draws);
        cap = std::max(cap, q.n);
        at[b] = {st.take(q.n, q.keys), st.take((size_t)q.n * 3, q.pos), st.take(q.nlevels, q.sigma2),
                 st.take(q.n, q.valid), st.take(q.n, q.best_mask), st.take((size_t)q.n_draws * 4, q.draws)};
    }
    ctx_enter(ctx);
    const PnpLayout L = pnp_layout(Mmax, cap);
    int r = st.open((size_t)B * L.stride);
    if (r != ORBX_OK) return r;
    for (int b = 0; b < B; b++) {
        const orbx_pnp_query& q = qs[b];
        const Staged& a = at[b];
        PnpCand& d = st.host(cands)[b];
        d.keys = st.dev(a.keys);
        d.match = nullptr;
        d.pos = st.dev(a.pos);
        d.valid = st.dev(a.valid);
        d.mask_in = st.dev(a.mask);
        d.sigma2 = st.dev(a.sigma2);
        d.draws = st.dev(a.draws);
        d.tab_min = d.tab_its = d.n_matches = nullptr;
        d.n = q.n;
        d.n2 = 0;
        d.nlevels = q.nlevels;
        ransac_parameters(Ns[b], q.probability, q.min_inliers, q.max_iterations, q.min_set, q.epsilon, &d.min_inl,
                          &d.max_its);
        d.min_matches = 0;
        d.iter_done = q.iter_done;
        d.best_in = q.best_inliers;
        d.n_iter = q.n_iter;
        d.n_draws = q.n_draws;
        d.th2 = q.th2;
        std::memcpy(d.cam, q.cam, 16);
        std::memcpy(d.Tcw_in, q.best_Tcw, 64);
    }
    ResultBlocks res(ctx, st.behind(), B, L.stride);
    if ((r = st.upload()) != ORBX_OK || (r = res.zero()) != ORBX_OK) return r;
    if ((r = launch_pnp(ctx, B, st.dev(cands), res.dev, L)) != ORBX_OK) return r;
    if ((r = res.read(read_bytes(L, B, qs))) != ORBX_OK) return r;
    for (int b = 0; b < B; b++) scatter(res.block(b), L, qs[b].n, &qs[b]);
    return ORBX_OK;
}

extern "C" int orbx_pnp_ransac(orbx_ctx* ctx, orbx_pnp_query* q) { return orbx_pnp_ransac_batch(ctx, 1, q); }

extern "C" int orbx_dev_pnp_candidates(orbx_ctx* ctx, int slot, int n, const orbx_bow_view* KFs,
                                       const float* const* pos, const float* cam, const float* sigma2, int nlevels,
                                       float nnratio, int check_ori, int min_matches, int32_t* const* matches_f,
                                       int cap, int* n_matches, int* discarded, orbx_pnp_query* out)
{
    if (!ctx || n < 0) return ORBX_ERR_ARG;
    if (n == 0) return ORBX_OK;
    if (!KFs || !pos || !cam || !matches_f || !n_matches || !discarded || !out || min_matches < 0 ||
        nlevels != ctx->geom.nlevels || nlevels < 1 || nlevels > kMaxLevels || !sigma2_ok(sigma2, nlevels))
        return ORBX_ERR_ARG;
    int Mmax = 1;
    for (int k = 0; k < n; k++) {
        if (!pos[k] || !matches_f[k]) return ORBX_ERR_ARG;
        const int r = check_params(out[k]);
        if (r != ORBX_OK) return r;
        Mmax = std::max(Mmax, out[k].n_draws);
    }
    const int nf = ctx->bow_nf;
    if (nf > kMaxFeatures) return ORBX_ERR_UNSUPPORTED;
    for (int k = 0; k < n; k++)
        if (out[k].cap < nf) return ORBX_ERR_CAPACITY;
    const int len = std::max(nf, 1);
    const PnpLayout L = pnp_layout(Mmax, len);
    // what the solver adds to the search's upload: descriptors | sigma2 | per
    // candidate: positions, the incoming mask, draws, the two tables | result blocks
    struct Staged {
        Region<float> pos;
        Region<uint8_t> mask;
        Region<int32_t> draws, tab_min, tab_its;
    };
    std::vector<Staged> at(n);
    PackedStage st(ctx);
    const Region<PnpCand> cands = st.take<PnpCand>(n);
    const Region<float> sig = st.take(nlevels, sigma2);
    for (int k = 0; k < n; k++) {
        if (KFs[k].n < 0 || KFs[k].n > kMaxFeatures) return ORBX_ERR_UNSUPPORTED;
        at[k] = {st.take((size_t)KFs[k].n * 3, pos[k]), st.take<uint8_t>(len), st.take((size_t)out[k].n_draws * 4, out[k].draws),
                 st.take<int32_t>(kMaxFeatures + 1), st.take<int32_t>(kMaxFeatures + 1)};
        st.later(at[k].mask.part(0, nf), out[k].best_mask);   // nf of the len bytes
    }
    st.align_end(256);
    BowQueued q;
    int r = queue_bow_frame(ctx, slot, n, KFs, nnratio, check_ori, matches_f, cap, st.total + (size_t)n * L.stride, &q);
    if (r != ORBX_OK) return r;
    st.bind(q.extra);
    for (int k = 0; k < n; k++) {
        const orbx_pnp_query& p = out[k];
        const Staged& a = at[k];
        PnpCand& d = st.host(cands)[k];
        d.keys = q.k1;
        d.match = q.out[k];
        d.valid = q.mp2[k];
        d.pos = st.dev(a.pos);
        d.mask_in = st.dev(a.mask);
        d.draws = st.dev(a.draws);
        for (int N = 0; N <= kMaxFeatures; N++)
            ransac_parameters(N, p.probability, p.min_inliers, p.max_iterations, p.min_set, p.epsilon,
                              &st.host(a.tab_min)[N], &st.host(a.tab_its)[N]);
        d.tab_min = st.dev(a.tab_min);
        d.tab_its = st.dev(a.tab_its);
        d.sigma2 = st.dev(sig);
        d.n_matches = q.out_n[k];
        d.n = nf;
        d.n2 = KFs[k].n;
        d.nlevels = nlevels;
        d.min_inl = d.max_its = 0;
        d.min_matches = min_matches;
        d.iter_done = p.iter_done;
        d.best_in = p.best_inliers;
        d.n_iter = p.n_iter;
        d.n_draws = p.n_draws;
        d.th2 = p.th2;
        std::memcpy(d.cam, cam, 16);
        std::memcpy(d.Tcw_in, p.best_Tcw, 64);
    }
    ResultBlocks res(ctx, st.behind(), n, L.stride);
    if ((r = st.upload()) != ORBX_OK || (r = res.zero()) != ORBX_OK) return r;
    if ((r = launch_pnp(ctx, n, st.dev(cands), res.dev, L)) != ORBX_OK) return r;
    if ((r = read_bow_queued(ctx, q, q.out_len, matches_f, n_matches)) != ORBX_OK) return r;
    if ((r = res.read(read_bytes(L, n, out))) != ORBX_OK) return r;
    for (int k = 0; k < n; k++) {
        if (n_matches[k] < 0) return ORBX_ERR_UNSUPPORTED;
        const uint8_t* blk = res.block(k);
        discarded[k] = reinterpret_cast<const PnpHdr*>(blk)->discarded;
        scatter(blk, L, nf, &out[k]);
    }
    return ORBX_OK;
}
