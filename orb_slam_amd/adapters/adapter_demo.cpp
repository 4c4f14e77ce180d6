// Exercises the C++ adapter (orbx_adapters.hpp) the way ORB-SLAM's Tracking
// and LocalMapping would: extract two frames of a shifted synthetic image,
// SearchForInitialization between them, the initialisation models of those
// matches (Initializer::FindModels beside the plain C call fed the same rand()
// sequence), brute-force matching, and one local BA on a tiny synthetic problem.  Prints one JSON line.  Exit codes: 0 ok,
// 3 device path unavailable (orbx_error), 1 other failure.
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
        std::printf("{\"n1\": %zu, \"n2\": %zu, \"levels\": %d, \"scale\": %.3f, \"init_matches\": %d, "
                    "\"bf_matches\": %d, \"ba_iterations\": [%d, %d], \"ba_chi2\": [%.6g, %.6g], "
                    "\"pose_inliers\": %d, \"pose_edges\": %d, \"pose_tx\": %.6g, \"init_same\": %d, "
                    "\"init_n\": %d, \"init_best\": [%d, %d], \"init_rh\": %.6g, \"init_inliers\": [%d, %d]}\n",
                    F1.keys_un.size(), F2.keys_un.size(), ex.GetLevels(), ex.GetScaleFactor(), n_init, n_bf,
                    P.stats.iterations[0], P.stats.iterations[1], P.stats.chi2_initial[0], P.stats.chi2_final[1],
                    n_pose_inliers, n_mp, PF.Tcw[3], init_same ? 1 : 0, q.n_matches, q.best_h, q.best_f, (double)q.RH,
                    n_in_h, n_in_f);
        return 0;
    } catch (const orbx_error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
