// Exercises the C++ adapter (orbx_adapters.hpp) the way ORB-SLAM's Tracking
// and LocalMapping would: extract two frames of a shifted synthetic image,
// SearchForInitialization between them, the initialisation models of those
// matches (Initializer::FindModels beside the plain C call fed the same rand()
// sequence), the whole Initializer::Initialize beside orbx_init_reconstruct, brute-force matching, one local BA on a tiny synthetic problem, and
// Sim3Solver::iterate in chunks of five beside orbx_sim3_ransac fed the same rand() sequence, Optimizer::OptimizeSim3
// beside orbx_optimize_sim3.  Prints one JSON line.  Exit codes: 0 ok,
// 3 device path unavailable (orbx_error), 1 other failure.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbx_adapters.hpp"

using namespace ORB_SLAM_AMD;

static std::vector<uint8_t> make_image(int w, int h, int dx, uint32_t seed)
{
    // box-filtered LCG noise + rectangles, shifted by dx columns
    const int W = w + 64;
    std::vector<uint8_t> big((size_t)W * h);
    uint32_t s = seed;
    for (auto& v : big) {
        s = s * 1664525u + 1013904223u;
        v = (uint8_t)(s >> 24);
    }
    std::vector<uint8_t> sm(big.size());
    for (int y = 0; y < h; y++)
        for (int x = 0; x < W; x++) {
            int acc = 0, n = 0;
            for (int j = -2; j <= 2; j++)
                for (int i = -2; i <= 2; i++) {
                    const int yy = y + j, xx = x + i;
                    if (yy >= 0 && yy < h && xx >= 0 && xx < W) {
                        acc += big[(size_t)yy * W + xx];
                        n++;
                    }
                }
            sm[(size_t)y * W + x] = (uint8_t)(acc / n);
        }
    for (int r = 0; r < 120; r++) {
        s = s * 1664525u + 1013904223u;
        const int x0 = (int)(s % (uint32_t)(W - 40)), y0 = (int)((s >> 8) % (uint32_t)(h - 30));
        const uint8_t val = (uint8_t)(s >> 16);
        for (int y = y0; y < y0 + 24; y++)
            for (int x = x0; x < x0 + 36; x++) sm[(size_t)y * W + x] = val;
    }
    std::vector<uint8_t> img((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) img[(size_t)y * w + x] = sm[(size_t)y * W + x + dx];
    return img;
}

int main()
{
    try {
        const int w = 640, h = 480;
        ORBextractor ex(1000, 1.2f, 8, ORBextractor::FAST_SCORE, 20, w, h);
        FrameData F1, F2;
        for (FrameData* F : {&F1, &F2}) {
            const auto img = make_image(w, h, F == &F1 ? 0 : 2, 7);
            ex(img.data(), w, h, w, F->keys_un, F->desc);
            F->max_x = (float)w;
            F->max_y = (float)h;
        }
        ORBmatcher matcher(0.9f, true, ex.context());
        std::vector<Point2f> prev(F1.keys_un.size());
        for (size_t i = 0; i < prev.size(); i++) prev[i] = {F1.keys_un[i].x, F1.keys_un[i].y};
        std::vector<int> m12;
        const int n_init = matcher.SearchForInitialization(F1, F2, prev, m12, 100);
        // Initializer::Initialize's model searches on the matches just found
        Initializer initializer(F1.keys_un, 1.0f, 200, ex.context());
        std::vector<bool> inH, inF;
        float SH = 0.f, SF = 0.f, H[9] = {0}, Fm[9] = {0};
        std::srand(1);
        const float RH = initializer.FindModels(F2.keys_un, m12, inH, SH, H, inF, SF, Fm);
        // the C call, fed the rand() values the adapter drew
        std::srand(1);
        std::vector<int32_t> draws(200 * 8);
        for (auto& d : draws) d = (int32_t)std::rand();
        std::vector<int32_t> m12c(m12.begin(), m12.end());
        std::vector<uint8_t> cH(m12.size() + 1), cF(m12.size() + 1);
        orbx_init_query q;
        std::memset(&q, 0, sizeof(q));
        q.keys1 = F1.keys_un.data();
        q.n1 = (int)F1.keys_un.size();
        q.keys2 = F2.keys_un.data();
        q.n2 = (int)F2.keys_un.size();
        q.matches12 = m12c.data();
        q.sigma = 1.0f;
        q.max_iter = 200;
        q.draws = draws.data();
        q.inliers_h = cH.data();
        q.inliers_f = cF.data();
        q.cap = (int)m12.size();
        check(orbx_init_models(ex.context(), &q), "orbx_init_models");
        bool init_same = q.n_matches == n_init && q.best_h == initializer.mBestH && q.best_f == initializer.mBestF &&
                         std::memcmp(&q.SH, &SH, 4) == 0 && std::memcmp(&q.SF, &SF, 4) == 0 &&
                         std::memcmp(&q.RH, &RH, 4) == 0 && (int)inH.size() == q.n_matches;
        if (q.best_h >= 0) init_same = init_same && std::memcmp(q.H21, H, sizeof(H)) == 0;
        if (q.best_f >= 0) init_same = init_same && std::memcmp(q.F21, Fm, sizeof(Fm)) == 0;
        int n_in_h = 0, n_in_f = 0;
        for (int i = 0; i < q.n_matches && init_same; i++) {
            init_same = inH[i] == (cH[i] != 0) && inF[i] == (cF[i] != 0);
            n_in_h += cH[i];
            n_in_f += cF[i];
        }
        // Initializer::Initialize beside the plain C reconstruction fed the models just read
        const float K[9] = {500.f, 0.f, 320.f, 0.f, 500.f, 240.f, 0.f, 0.f, 1.f};
        float R21[9] = {0}, t21[3] = {0};
        std::vector<Point3f> vP3D;
        std::vector<bool> vbTri;
        std::srand(1);
        const bool init_ok = initializer.Initialize(F2.keys_un, m12, K, R21, t21, vP3D, vbTri);
        const float camK[4] = {K[0], K[4], K[2], K[5]};
        std::vector<float> p3d(F1.keys_un.size() * 3 + 3);
        std::vector<uint8_t> tri(F1.keys_un.size() + 1);
        orbx_reconstruct_query rq;
        std::memset(&rq, 0, sizeof(rq));
        rq.keys1 = q.keys1;
        rq.n1 = q.n1;
        rq.keys2 = q.keys2;
        rq.n2 = q.n2;
        rq.matches12 = q.matches12;
        rq.model = q.RH > 0.40 ? 0 : 1;
        rq.inliers = rq.model ? cF.data() : cH.data();
        rq.M21 = rq.model ? q.F21 : q.H21;
        rq.cam = camK;
        rq.sigma = 1.0f;
        rq.min_parallax = 1.0f;
        rq.min_triangulated = 50;
        rq.p3d = p3d.data();
        rq.triangulated = tri.data();
        rq.cap = rq.n1;
        bool rec_same = rq.model == initializer.mModel && vP3D.size() == F1.keys_un.size();
        int n_tri = 0;
        if ((rq.model ? q.best_f : q.best_h) >= 0) {
            check(orbx_init_reconstruct(ex.context(), &rq), "orbx_init_reconstruct");
            rec_same = rec_same && (rq.ok != 0) == init_ok && rq.best == initializer.mBestHypothesis;
            if (rq.ok) rec_same = rec_same && std::memcmp(rq.R21, R21, sizeof(R21)) == 0 && std::memcmp(rq.t21, t21, sizeof(t21)) == 0;
            for (int i = 0; i < rq.n1 && rec_same; i++) {
                rec_same = std::memcmp(&p3d[3 * i], &vP3D[i], 12) == 0 && vbTri[i] == (tri[i] != 0);
                n_tri += tri[i];
            }
        } else {
            rec_same = rec_same && !init_ok;
        }
        // an accepted pair: 240 points of a cloud 3-12 m away, projected before and after a sideways motion
        // (a rotation of 0.08 rad about y, t = (-0.6, 0.05, 0.1)), keypoint i matched with keypoint i
        std::vector<KeyPoint> sk1, sk2;
        std::vector<int> sm;
        const double ang = 0.08, ca = std::cos(ang), sa = std::sin(ang), tt[3] = {-0.6, 0.05, 0.1};
        uint32_t ls = 7;
        auto rnd = [&ls]() {
            ls = ls * 1664525u + 1013904223u;
            return (double)(ls >> 8) / 16777216.0;
        };
        for (int i = 0; i < 240; i++) {
            const double u = 20.0 + 600.0 * rnd(), v = 20.0 + 440.0 * rnd(), z = 3.0 + 9.0 * rnd();
            const double X = (u - 320.0) / 500.0 * z, Y = (v - 240.0) / 500.0 * z;
            const double xc = ca * X + sa * z + tt[0], yc = Y + tt[1], zc = -sa * X + ca * z + tt[2];
            KeyPoint a;
            std::memset(&a, 0, sizeof(a));
            a.size = 31.f;
            a.class_id = -1;
            KeyPoint b = a;
            a.x = (float)u;
            a.y = (float)v;
            b.x = (float)(500.0 * xc / zc + 320.0);
            b.y = (float)(500.0 * yc / zc + 240.0);
            sk1.push_back(a);
            sk2.push_back(b);
            sm.push_back(i);
        }
        Initializer scene_init(sk1, 1.0f, 200, ex.context());
        float sR[9] = {0}, st[3] = {0};
        std::vector<Point3f> sP3D;
        std::vector<bool> sTri;
        std::srand(2);
        const bool scene_ok = scene_init.Initialize(sk2, sm, K, sR, st, sP3D, sTri);
        int scene_tri = 0, scene_front = 0;
        for (size_t i = 0; i < sTri.size(); i++)
            if (sTri[i]) {
                scene_tri++;
                scene_front += sP3D[i].z > 0.f;
            }
        // the recovered translation is the true one up to scale, the rotation the true one
        const double tn = std::sqrt(tt[0] * tt[0] + tt[1] * tt[1] + tt[2] * tt[2]);
        const double t_cos = scene_ok ? (st[0] * tt[0] + st[1] * tt[1] + st[2] * tt[2]) / tn : 0.0;
        const double r_trace = scene_ok ? (sR[0] * ca + sR[2] * sa + sR[4] - sR[6] * sa + sR[8] * ca) : 0.0;
        // Sim3Solver on a synthetic pair of maps: 80 points seen by both keyframes, the second map a similarity of
        // the first (scale 1.25), every fifth partner unrelated; iterate(5) until it returns, as ComputeSim3 does,
        // beside the plain C call fed the same rand() sequence
        Sim3KeyFrame sk[2];
        const double s_true = 1.25, sang = 0.1, sca = std::cos(sang), ssa = std::sin(sang), stt[3] = {0.3, -0.2, 0.4};
        for (int i = 0; i < 80; i++) {
            const double X2[3] = {-2.0 + 4.0 * rnd(), -1.5 + 3.0 * rnd(), 4.0 + 5.0 * rnd()};
            double X1[3] = {s_true * (sca * X2[0] + ssa * X2[2]) + stt[0], s_true * X2[1] + stt[1],
                            s_true * (-ssa * X2[0] + sca * X2[2]) + stt[2]};
            if (i % 5 == 4) X1[0] += 1.0 + rnd();
            KeyPoint kp;
            std::memset(&kp, 0, sizeof(kp));
            kp.size = 31.f;
            kp.class_id = -1;
            for (int side = 0; side < 2; side++) {
                kp.octave = (i + 3 * side) % 8;
                sk[side].keys.push_back(kp);
                const double* X = side ? X2 : X1;
                sk[side].pos.insert(sk[side].pos.end(), {(float)X[0], (float)X[1], (float)X[2]});
                sk[side].valid.push_back(1);
            }
        }
        for (int side = 0; side < 2; side++) {
            const float I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            std::memcpy(sk[side].Tcw, I4, sizeof(I4));
            std::memcpy(sk[side].cam, camK, sizeof(camK));
            float lv = 1.f;
            for (int l = 0; l < 8; l++, lv *= 1.2f) sk[side].sigma2.push_back(lv * lv);
        }
        std::vector<int> sim3_m(80);
        for (int i = 0; i < 80; i++) sim3_m[i] = i;
        Sim3Solver solver(sk[0], sk[1], sim3_m, ex.context());
        solver.SetRansacParameters(0.99, 20, 300);
        std::srand(1);
        bool sim3_no_more = false;
        std::vector<bool> sim3_inl;
        int sim3_n_inl = 0, sim3_calls = 0;
        std::vector<float> sim3_T;
        while (sim3_T.empty() && !sim3_no_more) {
            sim3_T = solver.iterate(5, sim3_no_more, sim3_inl, sim3_n_inl);
            sim3_calls++;
        }
        std::srand(1);
        std::vector<int32_t> sim3_m32(sim3_m.begin(), sim3_m.end()), sim3_draws(15);
        std::vector<uint8_t> sim3_ci(81);
        orbx_sim3_query sq;
        std::memset(&sq, 0, sizeof(sq));
        sq.keys1 = sk[0].keys.data();
        sq.keys2 = sk[1].keys.data();
        sq.n1 = sq.n2 = 80;
        sq.matches12 = sim3_m32.data();
        sq.pos1 = sk[0].pos.data();
        sq.pos2 = sk[1].pos.data();
        sq.valid1 = sk[0].valid.data();
        sq.valid2 = sk[1].valid.data();
        sq.T1w = sk[0].Tcw;
        sq.T2w = sk[1].Tcw;
        sq.cam1 = sk[0].cam;
        sq.cam2 = sk[1].cam;
        sq.sigma2_1 = sk[0].sigma2.data();
        sq.sigma2_2 = sk[1].sigma2.data();
        sq.nlevels = 8;
        sq.probability = 0.99;
        sq.min_inliers = 20;
        sq.max_iterations = 300;
        sq.n_iter = 5;
        sq.draws = sim3_draws.data();
        sq.inliers = sim3_ci.data();
        sq.cap = 80;
        int sim3_ccalls = 0;
        do {
            for (auto& d : sim3_draws) d = (int32_t)std::rand();
            check(orbx_sim3_ransac(ex.context(), &sq), "orbx_sim3_ransac");
            sq.iter_done += sq.iters_run;
            sq.best_inliers = sq.best_inliers_out;
            sim3_ccalls++;
        } while (!sq.found && !sq.no_more);
        bool sim3_same = sim3_ccalls == sim3_calls && (sq.found != 0) == !sim3_T.empty() && sq.n_inliers == sim3_n_inl &&
                         sq.iter_done == solver.mnIterations && sq.N == solver.N && (int)sim3_inl.size() == 80;
        if (sq.found && sim3_same)
            sim3_same = std::memcmp(sq.T12, sim3_T.data(), sizeof(sq.T12)) == 0 &&
                        std::memcmp(sq.R12, solver.GetEstimatedRotation(), sizeof(sq.R12)) == 0 &&
                        std::memcmp(sq.t12, solver.GetEstimatedTranslation(), sizeof(sq.t12)) == 0 &&
                        sq.s12 == solver.GetEstimatedScale();
        for (int i = 0; i < 80 && sim3_same; i++) sim3_same = sim3_inl[i] == (sim3_ci[i] != 0);
        // Optimizer::OptimizeSim3 on the same pair, started from the solver's estimate as ComputeSim3 does
        // (src/LoopClosing.cc:324-328): the keypoints at the projections of each keyframe's own points, so the 64
        // true pairs fit and the 16 unrelated ones are gross; the adapter beside the plain C call
        Sim3KeyFrame ok[2] = {sk[0], sk[1]};
        for (int side = 0; side < 2; side++)
            for (int i = 0; i < 80; i++) {
                const float* X = &ok[side].pos[3 * i];
                ok[side].keys[i].x = camK[0] * X[0] / X[2] + camK[2];
                ok[side].keys[i].y = camK[1] * X[1] / X[2] + camK[3];
            }
        std::vector<int> opt_m(sim3_m);
        opt_m[7] = -2;    // a point KF2 does not observe: skipped and left as it is
        Sim3 gS12(sq.R12, sq.t12, sq.s12);
        const int opt_n_in = Optimizer::OptimizeSim3(ex.context(), ok[0], ok[1], opt_m, gS12, 10.f);
        const Sim3 gProduct = gS12 * Sim3();   // gScm * gSmw with an identity: the same transformation
        std::vector<int32_t> opt_m32(sim3_m.begin(), sim3_m.end());
        opt_m32[7] = -2;
        std::vector<float> opt_inv;
        for (float v : ok[0].sigma2) opt_inv.push_back(1.0f / v);
        orbx_sim3_opt_query oq;
        std::memset(&oq, 0, sizeof(oq));
        oq.keys1 = ok[0].keys.data();
        oq.keys2 = ok[1].keys.data();
        oq.n1 = oq.n2 = 80;
        oq.matches12 = opt_m32.data();
        oq.pos1 = ok[0].pos.data();
        oq.pos2 = ok[1].pos.data();
        oq.valid1 = ok[0].valid.data();
        oq.valid2 = ok[1].valid.data();
        oq.T1w = ok[0].Tcw;
        oq.T2w = ok[1].Tcw;
        oq.cam1 = ok[0].cam;
        oq.cam2 = ok[1].cam;
        oq.inv_sigma2_1 = opt_inv.data();
        oq.sigma2_2 = ok[1].sigma2.data();
        oq.nlevels = 8;
        std::memcpy(oq.R12, sq.R12, sizeof(oq.R12));
        std::memcpy(oq.t12, sq.t12, sizeof(oq.t12));
        oq.s12 = sq.s12;
        oq.th2 = 10.f;
        check(orbx_optimize_sim3(ex.context(), &oq), "orbx_optimize_sim3");
        bool sim3opt_same = oq.n_in == opt_n_in && !oq.returned_early && opt_m[7] == -2 &&
                            std::memcmp(oq.q12, gS12.q, sizeof(oq.q12)) == 0 &&
                            std::memcmp(oq.t12d, gS12.t, sizeof(oq.t12d)) == 0 && oq.s12d == gS12.s &&
                            std::memcmp(gProduct.q, gS12.q, sizeof(gS12.q)) == 0 && gProduct.s == gS12.s;
        for (int i = 0; i < 80 && sim3opt_same; i++) sim3opt_same = opt_m[i] == opt_m32[i];
        // PnPsolver on a synthetic frame: 80 keypoints with a map point each, seen from a known pose, every fifth
        // partner unrelated; iterate(5) as Relocalisation drives it until it returns, beside the plain C call fed
        // the same rand() sequence
        PnPFrame pf;
        std::memcpy(pf.cam, camK, sizeof(camK));
        {
            float lv = 1.f;
            for (int l = 0; l < 8; l++, lv *= 1.2f) pf.sigma2.push_back(lv * lv);
        }
        std::vector<float> pnp_pos;
        std::vector<uint8_t> pnp_valid;
        const double pang = 0.15, pca = std::cos(pang), psa = std::sin(pang), ptt[3] = {0.2, -0.1, 0.3};
        for (int i = 0; i < 80; i++) {
            const double Xc[3] = {-2.0 + 4.0 * rnd(), -1.5 + 3.0 * rnd(), 4.0 + 5.0 * rnd()};
            // Xc = R Xw + t with R a rotation about y: Xw = R^T (Xc - t)
            const double dx = Xc[0] - ptt[0], dy = Xc[1] - ptt[1], dz = Xc[2] - ptt[2];
            double Xw[3] = {pca * dx - psa * dz, dy, psa * dx + pca * dz};
            if (i % 5 == 4) Xw[0] += 1.0 + rnd();
            KeyPoint kp;
            std::memset(&kp, 0, sizeof(kp));
            kp.x = (float)(camK[0] * Xc[0] / Xc[2] + camK[2]);
            kp.y = (float)(camK[1] * Xc[1] / Xc[2] + camK[3]);
            kp.size = 31.f;
            kp.class_id = -1;
            kp.octave = i % 8;
            pf.keys.push_back(kp);
            pnp_pos.insert(pnp_pos.end(), {(float)Xw[0], (float)Xw[1], (float)Xw[2]});
            pnp_valid.push_back(1);
        }
        PnPsolver pnp(pf, pnp_pos, pnp_valid, ex.context());
        pnp.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
        std::srand(1);
        bool pnp_no_more = false;
        std::vector<bool> pnp_inl;
        int pnp_n_inl = 0, pnp_calls = 0;
        std::vector<float> pnp_T;
        while (pnp_T.empty() && !pnp_no_more) {
            pnp_T = pnp.iterate(5, pnp_no_more, pnp_inl, pnp_n_inl);
            pnp_calls++;
        }
        std::srand(1);
        std::vector<uint8_t> pnp_ci(81), pnp_mask(81);
        std::vector<int32_t> pnp_draws;
        orbx_pnp_query pq;
        std::memset(&pq, 0, sizeof(pq));
        pq.keys = pf.keys.data();
        pq.n = 80;
        pq.pos = pnp_pos.data();
        pq.valid = pnp_valid.data();
        pq.cam = pf.cam;
        pq.sigma2 = pf.sigma2.data();
        pq.nlevels = 8;
        pq.probability = 0.99;
        pq.min_inliers = 10;
        pq.max_iterations = 300;
        pq.min_set = 4;
        pq.epsilon = 0.5f;
        pq.th2 = 5.991f;
        pq.n_iter = 5;
        pq.best_mask = pnp_mask.data();
        pq.inliers = pnp_ci.data();
        pq.cap = 80;
        int pnp_ccalls = 0;
        do {
            // as the adapter draws: four values for each iteration the call can run, zeros up to the required length
            const int pnp_can_run = std::max(5, pnp.mRansacMaxIts - pq.iter_done);
            pq.n_draws = std::max(5, 300 - pq.iter_done);
            pnp_draws.assign((size_t)pq.n_draws * 4, 0);
            for (int i = 0; i < pnp_can_run * 4; i++) pnp_draws[i] = (int32_t)std::rand();
            pq.draws = pnp_draws.data();
            check(orbx_pnp_ransac(ex.context(), &pq), "orbx_pnp_ransac");
            pnp_ccalls++;
        } while (!pq.found && !pq.no_more);
        bool pnp_same = pnp_ccalls == pnp_calls && (pq.found != 0) == !pnp_T.empty() && pq.n_inliers == pnp_n_inl &&
                        pq.iter_done == pnp.mnIterations && pq.best_inliers == pnp.mnBestInliers && pq.N == pnp.N;
        if (pq.found && pnp_same)
            pnp_same = (int)pnp_inl.size() == 80 && std::memcmp(pq.Tcw, pnp_T.data(), sizeof(pq.Tcw)) == 0 &&
                       std::memcmp(pq.best_Tcw, pnp.mBestTcw, sizeof(pq.best_Tcw)) == 0;
        for (int i = 0; i < 80 && pnp_same && pq.found; i++)
            pnp_same = pnp_inl[i] == (pnp_ci[i] != 0) && pnp.mvbBestInliers[i] == pnp_mask[i];
        // the returned pose against the true one
        double pnp_err = 0.0;
        if (pq.found) {
            const double Rt[9] = {pca, 0.0, psa, 0.0, 1.0, 0.0, -psa, 0.0, pca};
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) pnp_err = std::max(pnp_err, std::fabs((double)pq.Tcw[4 * r + c] - Rt[3 * r + c]));
                pnp_err = std::max(pnp_err, std::fabs((double)pq.Tcw[4 * r + 3] - ptt[r]));
            }
        }
        // find() where no Refine returns: every partner unrelated, so it runs mRansacMaxIts iterations (35 here,
        // not the 300 passed to SetRansacParameters) and returns nothing
        std::vector<float> pnp_pos2;
        for (int i = 0; i < 80; i++) pnp_pos2.insert(pnp_pos2.end(), {(float)(-3.0 + 6.0 * rnd()), (float)(-3.0 + 6.0 * rnd()), (float)(2.0 + 8.0 * rnd())});
        PnPsolver pnp2(pf, pnp_pos2, pnp_valid, ex.context());
        pnp2.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
        std::srand(3);
        std::vector<bool> pnp2_inl;
        int pnp2_n_inl = 0;
        const std::vector<float> pnp2_T = pnp2.find(pnp2_inl, pnp2_n_inl);
        std::vector<int> mbf;
        const int n_bf = matcher.MatchBruteForce(F1.desc, F2.desc, mbf);
        // tiny BA: 3 keyframes (first fixed) observing 60 points
        LocalBAProblem P;
        const int nk = 3, np = 60;
        for (int k = 0; k < nk; k++) {
            const double ang = 0.02 * k;
            P.pose_q.insert(P.pose_q.end(), {0.0, std::sin(ang / 2), 0.0, std::cos(ang / 2)});
            P.pose_t.insert(P.pose_t.end(), {-0.1 * k + (k ? 0.01 : 0.0), 0.0, 0.0});
            P.pose_fixed.push_back(k == 0);
            P.pose_id.push_back(k);
            P.pose_cam.insert(P.pose_cam.end(), {500.0, 500.0, 320.0, 240.0});
        }
        uint32_t s = 11;
        for (int p = 0; p < np; p++) {
            s = s * 1664525u + 1013904223u;
            const double X = ((s >> 8) % 2000) / 1000.0 - 1.0, Y = ((s >> 4) % 1500) / 1000.0 - 0.75,
                         Z = 3.0 + ((s >> 12) % 2000) / 1000.0;
            P.points.insert(P.points.end(), {X + 0.01, Y - 0.01, Z});
            P.point_id.push_back(nk + p);
            P.point_nobs.push_back(nk);
            for (int k = 0; k < nk; k++) {
                const double ang = 0.02 * k, c = std::cos(ang), sn = std::sin(ang);
                const double xc = c * X + sn * Z - 0.1 * k, yc = Y, zc = -sn * X + c * Z;
                P.edge_point.push_back(p);
                P.edge_pose.push_back(k);
                P.edge_obs.push_back(500.0 * xc / zc + 320.0);
                P.edge_obs.push_back(500.0 * yc / zc + 240.0);
                P.edge_inv_sigma2.push_back(1.0);
            }
        }
        Optimizer::LocalBundleAdjustment(ex.context(), P);
        // PoseOptimization of F2: every other keypoint gets a map point 3-5 m
        // in front of the identity camera; the initial pose is off by 2 cm
        PoseFrame PF;
        PF.keys_un = F2.keys_un;
        PF.fx = PF.fy = 500.f;
        PF.cx = 320.f;
        PF.cy = 240.f;
        float sc = 1.f;
        for (int l = 0; l < 8; l++, sc *= 1.2f) PF.inv_level_sigma2.push_back(1.f / (sc * sc));
        for (size_t i = 0; i < PF.keys_un.size(); i++) {
            const bool mp = (i % 2) == 0;
            PF.has_mp.push_back(mp);
            const float z = 3.f + (float)(i % 7) * 0.3f;
            PF.mp_xyz.insert(PF.mp_xyz.end(), {(PF.keys_un[i].x - 320.f) / 500.f * z,
                                               (PF.keys_un[i].y - 240.f) / 500.f * z, z});
        }
        PF.Tcw[3] = 0.02f;
        const int n_pose_inliers = Optimizer::PoseOptimization(ex.context(), PF);
        int n_mp = 0;
        for (uint8_t m : PF.has_mp) n_mp += m;
        // Optimizer::OptimizeEssentialGraph on a small loop: eight keyframes on an arc whose map grew by 3 % per
        // keyframe (pure scale drift), the last one closing onto the first.  CorrectLoop has given the current
        // keyframe its corrected Sim3 (the true pose at the drifted scale) and its pose the corrected SE3.  Through
        // the adapter (which builds the edge list) and through the plain C call on the adapter's edges
        EssentialGraph EG;
        const int eg_n = 8;
        double eg_scale7 = 1.0;
        for (int k = 0; k < eg_n; k++) {
            EssentialGraph::KeyFrame kf;
            kf.mnId = 10 + 2 * k;
            const double a = 0.4 * k, f = 1.0 + 0.03 * k;
            const double R[9] = {std::cos(a), 0, std::sin(a), 0, 1, 0, -std::sin(a), 0, std::cos(a)};
            const double c[3] = {3 * std::cos(a), 0.1 * k, 3 * std::sin(a)};
            float Rf[9], tf[3], tdrift[3];
            for (int i = 0; i < 3; i++) {
                const double t = -(R[3 * i] * c[0] + R[3 * i + 1] * c[1] + R[3 * i + 2] * c[2]);
                tf[i] = (float)t;
                tdrift[i] = (float)(f * t);
            }
            for (int i = 0; i < 9; i++) Rf[i] = (float)R[i];
            std::memcpy(kf.Tcw, Rf, sizeof(Rf));
            std::memcpy(kf.Tcw + 9, tdrift, sizeof(tdrift));
            if (k > 0) kf.parent = 10 + 2 * (k - 1);
            if (k > 1) kf.covisibles = {kf.mnId - 2, kf.mnId - 4};        // the parent is skipped, k - 2 makes an edge
            if (k + 1 < eg_n) kf.children = {kf.mnId + 2};
            if (k == eg_n - 1) {
                kf.hasCorrected = kf.hasNonCorrected = true;
                kf.nonCorrected = Sim3(Rf, tdrift, 1.f);
                kf.corrected = Sim3(Rf, tf, 1.f);
                for (int i = 0; i < 3; i++) kf.corrected.t[i] *= f;
                kf.corrected.s = eg_scale7 = f;
                std::memcpy(kf.Tcw + 9, tf, sizeof(tf));
            }
            EG.keyframes.push_back(kf);
        }
        EG.loopKF = 10;
        EG.curKF = 10 + 2 * (eg_n - 1);
        EG.loopConnections = {{EG.curKF, {{EG.loopKF, 30}, {12, 20}, {14, 150}}}};   // the first is exempt from minFeat
        for (int k = 0; k < 40; k++)
            EG.points.push_back({{0.1f * k, 0.5f, 4.f + 0.05f * k}, k % 7 == 3 ? -1 : (long long)(10 + 2 * (k % eg_n))});
        EssentialGraph EGc = EG;
        Optimizer::OptimizeEssentialGraph(ex.context(), EG);
        const std::vector<orbx_essgraph_edge> eg_edges = EGc.BuildEdges();
        std::vector<orbx_essgraph_kf> eg_kfs(eg_n);
        std::vector<float> eg_pos, eg_pos_out(3 * EGc.points.size()), eg_Tcw(12 * eg_n);
        std::vector<int32_t> eg_ref;
        for (int k = 0; k < eg_n; k++) {
            const EssentialGraph::KeyFrame& kf = EGc.keyframes[k];
            std::memset(&eg_kfs[k], 0, sizeof(eg_kfs[k]));
            eg_kfs[k].id = (int64_t)kf.mnId;
            std::memcpy(eg_kfs[k].Tcw, kf.Tcw, sizeof(kf.Tcw));
            eg_kfs[k].has_corrected = kf.hasCorrected;
            eg_kfs[k].has_noncorrected = kf.hasNonCorrected;
            for (int i = 0; i < 8; i++) {
                eg_kfs[k].corrected[i] = i < 4 ? kf.corrected.q[i] : i < 7 ? kf.corrected.t[i - 4] : kf.corrected.s;
                eg_kfs[k].noncorrected[i] =
                    i < 4 ? kf.nonCorrected.q[i] : i < 7 ? kf.nonCorrected.t[i - 4] : kf.nonCorrected.s;
            }
        }
        for (const EssentialGraph::MapPoint& mp : EGc.points) {
            eg_pos.insert(eg_pos.end(), mp.pos, mp.pos + 3);
            eg_ref.push_back(mp.refKF < 0 ? -1 : EGc.IndexOf((unsigned long)mp.refKF));
        }
        eg_pos_out = eg_pos;
        orbx_essgraph_query eq;
        std::memset(&eq, 0, sizeof(eq));
        eq.kfs = eg_kfs.data();
        eq.n_kf = eg_n;
        eq.loop_kf = 0;
        eq.cur_kf = eg_n - 1;
        eq.edges = eg_edges.data();
        eq.n_edges = (int)eg_edges.size();
        eq.pos = eg_pos.data();
        eq.ref_kf = eg_ref.data();
        eq.n_points = (int)eg_ref.size();
        eq.Tcw_out = eg_Tcw.data();
        eq.pos_out = eg_pos_out.data();
        check(orbx_optimize_essential_graph(ex.context(), &eq), "orbx_optimize_essential_graph");
        bool essgraph_same = eq.iterations == EG.iterations && eq.trials == EG.trials && eq.chi2_last == EG.chi2Last;
        for (int k = 0; k < eg_n && essgraph_same; k++)
            essgraph_same = std::memcmp(EG.keyframes[k].Tcw, &eg_Tcw[12 * k], 48) == 0;
        for (size_t k = 0; k < EG.points.size() && essgraph_same; k++)
            essgraph_same = std::memcmp(EG.points[k].pos, &eg_pos_out[3 * k], 12) == 0;
        // the loop closes: the recovered camera centre of the current keyframe against the true one (where the
        // corrected pose has it) and, for scale, the distance of the drifted centre from the true one
        auto centre = [](const float* T, double c[3]) {   // -R^T t
            for (int i = 0; i < 3; i++) c[i] = -((double)T[i] * T[9] + (double)T[3 + i] * T[10] + (double)T[6 + i] * T[11]);
        };
        double eg_c_true[3], eg_c_opt[3], essgraph_centre_err = 0, essgraph_centre_gap = 0;
        centre(EGc.keyframes[eg_n - 1].Tcw, eg_c_true);
        centre(EG.keyframes[eg_n - 1].Tcw, eg_c_opt);
        for (int i = 0; i < 3; i++) {
            essgraph_centre_err += (eg_c_opt[i] - eg_c_true[i]) * (eg_c_opt[i] - eg_c_true[i]);
            essgraph_centre_gap += (eg_scale7 - 1) * eg_c_true[i] * (eg_scale7 - 1) * eg_c_true[i];
        }
        essgraph_centre_err = std::sqrt(essgraph_centre_err);
        essgraph_centre_gap = std::sqrt(essgraph_centre_gap);
        std::printf("{\"n1\": %zu, \"n2\": %zu, \"levels\": %d, \"scale\": %.3f, \"init_matches\": %d, "
                    "\"bf_matches\": %d, \"ba_iterations\": [%d, %d], \"ba_chi2\": [%.6g, %.6g], "
                    "\"pose_inliers\": %d, \"pose_edges\": %d, \"pose_tx\": %.6g, \"init_same\": %d, "
                    "\"init_n\": %d, \"init_best\": [%d, %d], \"init_rh\": %.6g, \"init_inliers\": [%d, %d], "
                    "\"rec_same\": %d, \"rec_model\": %d, \"rec_ok\": %d, \"rec_hyp\": %d, \"rec_good\": %d, "
                    "\"rec_triangulated\": %d, \"scene_ok\": %d, \"scene_model\": %d, \"scene_triangulated\": %d, "
                    "\"scene_in_front\": %d, \"scene_t_cos\": %.6f, \"scene_r_trace\": %.6f, ",
                    F1.keys_un.size(), F2.keys_un.size(), ex.GetLevels(), ex.GetScaleFactor(), n_init, n_bf,
                    P.stats.iterations[0], P.stats.iterations[1], P.stats.chi2_initial[0], P.stats.chi2_final[1],
                    n_pose_inliers, n_mp, PF.Tcw[3], init_same ? 1 : 0, q.n_matches, q.best_h, q.best_f, (double)q.RH,
                    n_in_h, n_in_f, rec_same ? 1 : 0, rq.model, init_ok ? 1 : 0, rq.n_hyp,
                    rq.n_hyp > 0 && rq.best >= 0 ? rq.n_good[rq.best] : 0, n_tri, scene_ok ? 1 : 0, scene_init.mModel,
                    scene_tri, scene_front, t_cos, r_trace);
        std::printf("\"sim3_same\": %d, \"sim3_n\": %d, \"sim3_found\": %d, \"sim3_inliers\": %d, "
                    "\"sim3_iterations\": %d, \"sim3_scale\": %.6f, ",
                    sim3_same ? 1 : 0, sq.N, sq.found, sq.n_inliers, sq.iter_done, (double)solver.GetEstimatedScale());
        std::printf("\"sim3opt_same\": %d, \"sim3opt_n_in\": %d, \"sim3opt_n_corr\": %d, \"sim3opt_n_bad\": %d, "
                    "\"sim3opt_scale\": %.9f, ",
                    sim3opt_same ? 1 : 0, opt_n_in, oq.n_corr, oq.n_bad, gS12.s);
        std::printf("\"essgraph_same\": %d, \"essgraph_edges\": %d, \"essgraph_iterations\": %d, "
                    "\"essgraph_chi2\": [%.6g, %.6g], \"essgraph_centre_err\": %.4g, \"essgraph_centre_gap\": %.4g, "
                    "\"essgraph_scale\": [%.6f, %.6f], ",
                    essgraph_same ? 1 : 0, (int)eg_edges.size(), EG.iterations, EG.chi2First, EG.chi2Last,
                    essgraph_centre_err, essgraph_centre_gap, EG.optimised[eg_n - 1].s, eg_scale7);
        std::printf("\"pnp_same\": %d, \"pnp_n\": %d, \"pnp_found\": %d, \"pnp_refined\": %d, \"pnp_inliers\": %d, "
                    "\"pnp_iterations\": %d, \"pnp_calls\": %d, \"pnp_pose_error\": %.3g, \"pnp_max_its\": %d, "
                    "\"pnp_find_found\": %d, \"pnp_find_iterations\": %d, \"pnp_find_max_its\": %d, "
                    "\"pnp_find_best\": %d, ",
                    pnp_same ? 1 : 0, pq.N, pq.found, pq.refined, pq.n_inliers, pq.iter_done, pnp_ccalls, pnp_err,
                    pq.ransac_max_its == pnp.mRansacMaxIts ? pnp.mRansacMaxIts : -1, pnp2_T.empty() ? 0 : 1,
                    pnp2.mnIterations, pnp2.mRansacMaxIts, pnp2.mnBestInliers);
        // KeyFrameDatabase: four keyframes added in the order 9, 2, 7, 5, each sharing two of the query's four
        // words (every score 0.5); the sharing list goes by smallest common word, then add order: 7 5 2 9.
        // Erased and added again, 7 goes behind 5.  Then LoopClosing::DetectLoop's pair of calls in one: the
        // covisible 2 and 9 give minScore 0.5, the connected 5 is left out
        KeyFrameDatabase kfdb(ex.context(), 16, 8);
        const BowVector kq({10, 20, 30, 40}, {.25, .25, .25, .25});
        kfdb.add(9, BowVector({30, 40}, {.5, .5}));
        kfdb.add(2, BowVector({20, 40}, {.5, .5}));
        kfdb.add(7, BowVector({10, 40}, {.5, .5}));
        kfdb.add(5, BowVector({10, 30}, {.5, .5}));
        kfdb.SetBestCovisibles(9, {3});   // 3 is not in the database: skipped
        const std::vector<int> kf_reloc = kfdb.DetectRelocalisationCandidates(kq);
        kfdb.erase(7);
        kfdb.add(7, BowVector({10, 20}, {.5, .5}));
        const std::vector<int> kf_reloc2 = kfdb.DetectRelocalisationCandidates(kq);
        const std::vector<int> kf_loop = kfdb.DetectLoopCandidates(kq, std::vector<int>{2, 9}, std::vector<int>{5});
        const float kf_min = kfdb.mMinScore;
        const std::vector<int> kf_loop_hi = kfdb.DetectLoopCandidates(kq, 0.75f, std::vector<int>());
        const std::vector<float> kf_scores = kfdb.score(kq, {5, 9});
        kfdb.clear();
        auto digits = [](const std::vector<int>& v) {   // ids below 10, as one decimal number
            int d = 0;
            for (int x : v) d = d * 10 + x;
            return d;
        };
        std::printf("\"kfdb_reloc\": %d, \"kfdb_reloc_readded\": %d, \"kfdb_loop\": %d, \"kfdb_min_score\": %.6f, "
                    "\"kfdb_loop_above\": %zu, \"kfdb_score\": [%.6f, %.6f], \"kfdb_size_after_clear\": %d, ",
                    digits(kf_reloc), digits(kf_reloc2), digits(kf_loop), (double)kf_min, kf_loop_hi.size(),
                    (double)kf_scores[0], (double)kf_scores[1], kfdb.size());
        // CovisibilityGraph: four keyframes whose keys (the KeyFrame* stand-ins) run 2 < 4 < 3 < 1, updated in
        // the order 1, 2, 3, 4 with th = 2.  1 counts 2 three times, 3 twice and 4 once: its list is 2 3, its
        // set in key order 2 4 3.  4 counts 1 and 3 once each: the fallback is 3, the smaller key.  Then 4 gains
        // point 14 and counts 1 and 3 twice: new weights, so the lists of 1 and 3 are rebuilt in full, with the
        // larger key first among equal weights.
        CovisibilityGraph covis(ex.context(), 8, 64, 8);
        covis.AddKeyFrame(1, 400, {10, 11, 12, 13, 14, 15});
        covis.AddKeyFrame(2, 100, {10, 11, 12, 20, 21});
        covis.AddKeyFrame(3, 300, {13, 14, 20, 30});
        covis.AddKeyFrame(4, 200, {15, 30, 31});
        const std::vector<int> cv_fronts = covis.UpdateConnections(std::vector<int>{1, 2, 3}, 2);
        const bool cv_updated4 = covis.UpdateConnections(4, 2);
        const int cv_front4 = covis.mFront;
        const int cv_ordered1 = digits(covis.GetVectorCovisibleKeyFrames(1));
        const int cv_connected1 = digits(covis.GetConnectedKeyFrames(1));
        const int cv_weight14 = covis.GetWeight(1, 4), cv_weight24 = covis.GetWeight(2, 4);
        const int cv_best1 = digits(covis.GetBestCovisibilityKeyFrames(1, 1));
        const int cv_by_weight3 = digits(covis.GetCovisiblesByWeight(1, 3));       // weights 3 2: the first below 3
        const size_t cv_by_weight2 = covis.GetCovisiblesByWeight(1, 2).size();     // every weight >= 2: end(), empty
        covis.EraseMapPointMatch(4, 2);
        covis.AddMapPoint(4, 14, 2);
        covis.UpdateConnections(4, 2);
        const int cv_front4b = covis.mFront;
        const int cv_ordered1b = digits(covis.GetVectorCovisibleKeyFrames(1));
        const int cv_ordered3b = digits(covis.GetVectorCovisibleKeyFrames(3));
        const int cv_ordered4b = digits(covis.GetVectorCovisibleKeyFrames(4));
        // a frame that sees 10, 20 twice and 30: 2 and 3 get three votes, 2 comes first in key order
        const CovisibilityGraph::Reference cv_ref = covis.UpdateReference({10, 20, 20, 30});
        covis.EraseMapPoints({20});
        const CovisibilityGraph::Reference cv_ref2 = covis.UpdateReference({10, 20, 20, 30});
        covis.EraseKeyFrame(2);   // EraseConnection on 1 and 3
        const int cv_ordered1c = digits(covis.GetVectorCovisibleKeyFrames(1));
        kfdb.add(1, BowVector({10, 40}, {.5, .5}));
        covis.PushBestCovisibles(kfdb, 1);
        std::printf("\"covis_fronts\": %d, \"covis_updated4\": %d, \"covis_front4\": %d, \"covis_ordered1\": %d, "
                    "\"covis_connected1\": %d, \"covis_weights\": [%d, %d], \"covis_best1\": %d, "
                    "\"covis_by_weight3\": %d, \"covis_by_weight2_size\": %zu, \"covis_front4_new\": %d, "
                    "\"covis_ordered1_new\": %d, \"covis_ordered3_new\": %d, \"covis_ordered4_new\": %d, "
                    "\"covis_local_kf\": %d, \"covis_ref_kf\": %d, \"covis_voters\": %d, \"covis_local_mp\": %d, "
                    "\"covis_local_mp_n\": %zu, \"covis_frame_erased\": %d, \"covis_ref_kf_after\": %d, "
                    "\"covis_ordered1_after_erase\": %d, \"covis_size\": %d, ",
                    digits(cv_fronts), cv_updated4 ? 1 : 0, cv_front4, cv_ordered1, cv_connected1, cv_weight14,
                    cv_weight24, cv_best1, cv_by_weight3, cv_by_weight2, cv_front4b, cv_ordered1b, cv_ordered3b,
                    cv_ordered4b, digits(cv_ref.mvpLocalKeyFrames), cv_ref.mpReferenceKF, cv_ref.nVoters,
                    cv_ref.mvpLocalMapPoints.empty() ? -1 : cv_ref.mvpLocalMapPoints.back(),
                    cv_ref.mvpLocalMapPoints.size(),
                    digits(std::vector<int>(cv_ref2.vbErased.begin(), cv_ref2.vbErased.end())), cv_ref2.mpReferenceKF,
                    cv_ordered1c, covis.size());
        // LocalMapping's culling.  Keyframes 0, 2, 3, 4 and 5 hold points 10..19; 2, 4 and 5 hold 50 as well, 5
        // also 60.  The tree is 0 <- 2 <- {3, 4}, 4 <- 5.  KeyFrameCulling(5) walks 4, 2, 3, 0 (weights 11, 11,
        // 10, 10, the larger key first).  4: ten of eleven points have three other observers, 10 > 9.9, but
        // LoopClosing holds it.  2: the same, culled; 50 is left with 4 and 5 and goes bad; 3 takes the parent 0
        // (weight 10, the first in key order), then 4 takes 3.  3: 0, 4 and 5 still see its ten points, culled;
        // 4 takes 0.  0 is skipped.  MapPointCulling(5): 10 stays, 60 was found once in five frames, 50 is bad.
        CovisibilityGraph lm(ex.context(), 8, 64, 16);
        const std::vector<int> shared = {10, 11, 12, 13, 14, 15, 16, 17, 18, 19};
        for (int id : {0, 2, 3, 4, 5}) {
            std::vector<int> row = shared;
            if (id == 2 || id == 4 || id == 5) row.push_back(50);
            if (id == 5) row.push_back(60);
            lm.AddKeyFrame(id, 100 * (uint64_t)id + 7, row);
            lm.SetOctaves(id, std::vector<int>(row.size(), 0));
            lm.UpdateConnections(id, 1);
        }
        lm.ChangeParent(2, 0);
        lm.ChangeParent(3, 2);
        lm.ChangeParent(4, 2);
        lm.ChangeParent(5, 4);
        const int lm_list5 = digits(lm.GetVectorCovisibleKeyFrames(5));
        const CovisibilityGraph::Culling lm_cull = lm.KeyFrameCulling(5, {4});
        std::list<CovisibilityGraph::RecentMapPoint> lm_recent = {{10, 5, 5, 3}, {60, 1, 5, 5}, {50, 4, 4, 4}};
        const std::vector<int> lm_bad = lm.MapPointCulling(5, lm_recent);
        std::printf("\"cull_list5\": %d, \"cull_culled\": %d, \"cull_to_be_erased\": %d, \"cull_bad_points\": %d, "
                    "\"cull_parents\": [%d, %d, %d], \"cull_childs0\": %d, \"cull_size\": %d, \"cull_mp_bad\": %d, "
                    "\"cull_mp_left\": %d, \"cull_mp_left_n\": %zu}\n",
                    lm_list5, digits(lm_cull.vpCulled), digits(lm_cull.vpToBeErased), digits(lm_cull.vpBadMapPoints),
                    lm.GetParent(3), lm.GetParent(4), lm.GetParent(5), digits(lm.GetChilds(0)), lm.size(),
                    digits(lm_bad), lm_recent.empty() ? -1 : lm_recent.front().mnId, lm_recent.size());
        return 0;
    } catch (const orbx_error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
