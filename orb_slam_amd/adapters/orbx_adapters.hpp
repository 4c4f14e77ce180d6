// C++ adapter over the orbx C ABI (include/orbx.h) that keeps the reference's
// class and function signatures for the hot path, so ORB-SLAM's callers
// (Frame, Tracking, LocalMapping) need only a type swap.  OpenCV-free: images
// are (pointer, w, h, stride) and descriptors N x 32 byte buffers; the
// cv::Mat glue a maintainer adds inside the reference is in INTEGRATION.md.
//
//   ORB_SLAM_AMD::ORBextractor   <- ORB_SLAM::ORBextractor   include/ORBextractor.h:32-77
//   ORB_SLAM_AMD::ORBmatcher     <- ORB_SLAM::ORBmatcher     include/ORBmatcher.h:37-107
//   ORB_SLAM_AMD::Optimizer      <- ORB_SLAM::Optimizer::LocalBundleAdjustment, PoseOptimization, OptimizeSim3,
//                                   OptimizeEssentialGraph
//                                                           include/Optimizer.h:42
//   ORB_SLAM_AMD::Initializer    <- ORB_SLAM::Initializer    include/Initializer.h:33-96
//                                   (FindHomography + FindFundamental)
//   ORB_SLAM_AMD::KeyFrameDatabase <- ORB_SLAM::KeyFrameDatabase include/KeyFrameDatabase.h:42-66
//
// Error behaviour: the reference has no error codes.  Like the reference, an
// empty image returns without touching the outputs (src/ORBextractor.cc:
// 721-722); every other failure of the device path throws orbx_error (there
// is no CPU fallback).
#pragma once

#include <cstdint>
#include <climits>
#include <cstdlib>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <list>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/orbx.h"

namespace ORB_SLAM_AMD {

struct orbx_error : std::runtime_error {
    int code;
    orbx_error(int c, const char* where)
        : std::runtime_error(std::string(where) + ": orbx error " + std::to_string(c)), code(c) {}
};

inline void check(int code, const char* where)
{
    if (code != ORBX_OK) throw orbx_error(code, where);
}

using KeyPoint = orbx_keypoint;   // layout of cv::KeyPoint (28 bytes)

// One device context per calling thread (the reference gives each thread its
// own extractor / matcher instances).
class Context {
public:
    Context(int nfeatures, float scale_factor, int nlevels, int score_type, int fast_th, int max_w, int max_h,
            int max_batch = 1, int device = 0)
    {
        // a library of another ABI revision may have changed a signature this
        // header calls through (include/orbx.h, ORBX_ABI_VERSION)
        if (orbx_abi_version() != ORBX_ABI_VERSION) throw orbx_error(ORBX_ERR_UNSUPPORTED, "orbx_abi_version");
        check(orbx_create(&ctx_, device, nfeatures, scale_factor, nlevels, score_type, fast_th, max_w, max_h, max_batch),
              "orbx_create");
    }
    ~Context() { orbx_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    orbx_ctx* get() const { return ctx_; }

private:
    orbx_ctx* ctx_ = nullptr;
};

// ---------------------------------------------------------------------------
// ORBextractor (src/ORBextractor.cc:457-779)
// ---------------------------------------------------------------------------
class ORBextractor {
public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

    ORBextractor(int nfeatures = 1000, float scaleFactor = 1.2f, int nlevels = 8, int scoreType = FAST_SCORE,
                 int fastTh = 20, int max_w = 1920, int max_h = 1080, int device = 0)
        : nfeatures_(nfeatures), ctx_(nfeatures, scaleFactor, nlevels, scoreType, fastTh, max_w, max_h, 1, device)
    {
    }

    // operator()(image, mask, keypoints, descriptors): keypoints cleared and
    // filled; descriptors resized to N*32 bytes (released when N == 0).
    void operator()(const uint8_t* image, int w, int h, size_t stride, std::vector<KeyPoint>& keypoints,
                    std::vector<uint8_t>& descriptors)
    {
        if (image == nullptr || w == 0 || h == 0) return;   // :721-722
        keypoints.resize(nfeatures_);
        descriptors.resize((size_t)nfeatures_ * 32);
        int n = 0;
        check(orbx_extract(ctx_.get(), image, w, h, stride, keypoints.data(), descriptors.data(), nfeatures_, &n),
              "ORBextractor::operator()");
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);
    }

    // With a mask (any size / content): the reference builds mvMaskPyramid
    // from it (:792-812) but FAST never reads the cell mask (:601-613), so
    // the outputs are those of the unmasked call.
    void operator()(const uint8_t* image, int w, int h, size_t stride, const uint8_t* /*mask*/,
                    std::vector<KeyPoint>& keypoints, std::vector<uint8_t>& descriptors)
    {
        (*this)(image, w, h, stride, keypoints, descriptors);
    }

    int GetLevels() const { return orbx_get_levels(ctx_.get()); }
    float GetScaleFactor() const { return orbx_get_scale_factor(ctx_.get()); }
    std::vector<int> GetFeaturesPerLevel() const
    {
        std::vector<int> v(64);
        v.resize(orbx_get_features_per_level(ctx_.get(), v.data(), 64));
        return v;
    }
    orbx_ctx* context() const { return ctx_.get(); }
    // Match a reference binary built with FMA contraction (GCC -O3
    // -march=native on an FMA host; orbx_set_fp_contract).
    void SetFpContract(bool enable) { check(orbx_set_fp_contract(ctx_.get(), enable ? 1 : 0), "SetFpContract"); }
    // retainBest's std::nth_element as the libstdc++ the reference was built
    // against implements it: gcc48 = GCC 4.6 .. 4.8 (orbx_set_nth_pivot).
    // The constructor leaves the default, GCC 4.6 .. 4.8: the reference
    // documents Ubuntu 12.04 / 14.04 (README.md:46), whose OpenCV 2.4
    // packages were built with those compilers; SetNthElementEra(false)
    // matches an OpenCV built with GCC >= 4.9.
    void SetNthElementEra(bool gcc48)
    {
        check(orbx_set_nth_pivot(ctx_.get(), gcc48 ? ORBX_NTH_PIVOT_GCC48 : ORBX_NTH_PIVOT_GCC49), "SetNthElementEra");
    }

private:
    int nfeatures_;
    Context ctx_;
};

// ---------------------------------------------------------------------------
// Frame data the matchers read (Frame::mvKeysUn, mDescriptors, image bounds,
// scale pyramid: src/Frame.cc:59-122, 320-348).
// ---------------------------------------------------------------------------
struct FrameData {
    std::vector<KeyPoint> keys_un;
    std::vector<uint8_t> desc;   // N x 32
    float min_x = 0, max_x = 0, min_y = 0, max_y = 0;
    int nlevels = 8;
    float scale_factor = 1.2f;

    orbx_frame_view view() const
    {
        orbx_frame_view v;
        v.keys_un = keys_un.data();
        v.desc = desc.data();
        v.n = (int)keys_un.size();
        v.min_x = min_x;
        v.max_x = max_x;
        v.min_y = min_y;
        v.max_y = max_y;
        v.nlevels = nlevels;
        v.scale_factor = scale_factor;
        return v;
    }
};

struct Point2f {
    float x, y;
};

// ---------------------------------------------------------------------------
// ORBmatcher (src/ORBmatcher.cc): the searches on the per-frame hot path.
// ---------------------------------------------------------------------------
class ORBmatcher {
public:
    static const int TH_LOW = 50;
    static const int TH_HIGH = 100;
    static const int HISTO_LENGTH = 30;

    // The matcher needs a device context; share the extractor's or own one.
    explicit ORBmatcher(float nnratio = 0.6f, bool checkOri = true, orbx_ctx* ctx = nullptr)
        : mfNNratio(nnratio), mbCheckOrientation(checkOri), ctx_(ctx)
    {
        if (!ctx_) {
            own_.reset(new Context(1000, 1.2f, 8, 1, 20, 64, 64));
            ctx_ = own_->get();
        }
    }

    // :1794-1810
    static int DescriptorDistance(const uint8_t* a, const uint8_t* b) { return orbx_descriptor_distance(a, b); }

    // :598-713
    int SearchForInitialization(const FrameData& F1, const FrameData& F2, std::vector<Point2f>& vbPrevMatched,
                                std::vector<int>& vnMatches12, int windowSize = 10)
    {
        const orbx_frame_view v1 = F1.view(), v2 = F2.view();
        vnMatches12.assign(v1.n, -1);
        int n = 0;
        check(orbx_search_for_initialization(ctx_, &v1, &v2, reinterpret_cast<float*>(vbPrevMatched.data()),
                                             vnMatches12.data(), windowSize, mfNNratio, mbCheckOrientation, &n),
              "ORBmatcher::SearchForInitialization");
        return n;
    }

    // :409-516.  f1_has_mp[i1]: F1.mvpMapPoints[i1] set and not bad.
    // vnMatches21[i2]: F1 index whose map point F2 keypoint i2 received, or -1.
    int WindowSearch(const FrameData& F1, const FrameData& F2, int windowSize, const std::vector<uint8_t>& f1_has_mp,
                     std::vector<int>& vnMatches21, int minOctave = -1, int maxOctave = INT32_MAX)
    {
        const orbx_frame_view v1 = F1.view(), v2 = F2.view();
        vnMatches21.assign(v2.n, -1);
        int n = 0;
        check(orbx_window_search(ctx_, &v1, &v2, f1_has_mp.data(), windowSize, minOctave,
                                 maxOctave == INT32_MAX ? -1 : maxOctave, mfNNratio, mbCheckOrientation,
                                 vnMatches21.data(), &n),
              "ORBmatcher::WindowSearch");
        return n;
    }

    // :49-125, local-map tracking (per map point: in_view, projection,
    // predicted level, viewing cosine, descriptor).
    int SearchByProjection(const FrameData& F, int n_mp, const uint8_t* in_view, const float* proj_xy,
                           const int32_t* pred_level, const float* view_cos, const uint8_t* mp_desc,
                           const uint8_t* f_assigned, float th, std::vector<int>& matches_f)
    {
        const orbx_frame_view v = F.view();
        matches_f.assign(v.n, -1);
        int n = 0;
        check(orbx_search_by_projection_local(ctx_, &v, n_mp, in_view, proj_xy, pred_level, view_cos, mp_desc,
                                              f_assigned, th, mfNNratio, matches_f.data(), &n),
              "ORBmatcher::SearchByProjection(local map)");
        return n;
    }

    // Tracking::SearchReferencePointsInFrustum (src/Tracking.cc:701-752):
    // Frame::isInFrustum for every local map point, then the local-map search
    // above, both on the device (no host pass over the local map).  The
    // per-point frustum results come back for IncreaseVisible() and the
    // MapPoint tracking fields; q.frame / q.matches_f are set here.
    int SearchLocalMap(const FrameData& F, orbx_local_map_query& q, std::vector<int>& matches_f)
    {
        const orbx_frame_view v = F.view();
        matches_f.assign(v.n, -1);
        q.frame = &v;
        q.matches_f = matches_f.data();
        q.nnratio = mfNNratio;
        check(orbx_search_local_map(ctx_, &q), "Tracking::SearchReferencePointsInFrustum");
        q.frame = nullptr;
        q.matches_f = nullptr;
        return q.n_matches;
    }

    // :1507-1620, motion-model tracking.
    int SearchByProjection(const FrameData& Cur, const FrameData& Last, const float* last_mp_xyz,
                           const uint8_t* last_mp_valid, const uint8_t* cur_assigned, const float* Tcw,
                           const float* cam, float th, std::vector<int>& matches_cur)
    {
        const orbx_frame_view vc = Cur.view(), vl = Last.view();
        matches_cur.assign(vc.n, -1);
        int n = 0;
        check(orbx_search_by_projection_motion(ctx_, &vc, &vl, last_mp_xyz, last_mp_valid, cur_assigned, Tcw, cam, th,
                                               mbCheckOrientation, matches_cur.data(), &n),
              "ORBmatcher::SearchByProjection(motion)");
        return n;
    }

    // :519-594, refinement after pose optimisation.
    int SearchByProjection(const FrameData& F1, const FrameData& F2, int windowSize, const float* f1_mp_xyz,
                           const uint8_t* f1_mp_valid, const uint8_t* f2_assigned, const float* Tcw2,
                           const float* cam, std::vector<int>& matches21)
    {
        const orbx_frame_view v1 = F1.view(), v2 = F2.view();
        matches21.assign(v2.n, -1);
        int n = 0;
        check(orbx_search_by_projection_pair(ctx_, &v1, &v2, f1_mp_xyz, f1_mp_valid, f2_assigned, Tcw2, cam,
                                             windowSize, mfNNratio, matches21.data(), &n),
              "ORBmatcher::SearchByProjection(pair)");
        return n;
    }

    // Brute-force matching of two descriptor sets (config C3: the B3 rule over
    // all pairs).
    int MatchBruteForce(const std::vector<uint8_t>& dA, const std::vector<uint8_t>& dB, std::vector<int>& m12,
                        int th_low = TH_LOW)
    {
        const int nA = (int)(dA.size() / 32), nB = (int)(dB.size() / 32);
        m12.assign(nA, -1);
        int n = 0;
        check(orbx_match_bf(ctx_, dA.data(), nA, dB.data(), nB, th_low, mfNNratio, m12.data(), &n),
              "ORBmatcher::MatchBruteForce");
        return n;
    }

    float mfNNratio;
    bool mbCheckOrientation;

private:
    orbx_ctx* ctx_;
    std::unique_ptr<Context> own_;
};

// ---------------------------------------------------------------------------
// Optimizer::LocalBundleAdjustment (src/Optimizer.cc:287-536).  The caller
// packs the local window (local keyframes, fixed covisible keyframes, local
// map points and their observations, in g2o insertion order) into a
// LocalBAProblem, runs it, then applies the results the way the reference
// does: erase the observations flagged in edge_status, write poses/points
// back for keyframes and non-bad points.
// ---------------------------------------------------------------------------
struct LocalBAProblem {
    std::vector<double> pose_q, pose_t, pose_cam, points, edge_obs, edge_inv_sigma2;
    std::vector<uint8_t> pose_fixed;
    std::vector<int64_t> pose_id, point_id;
    std::vector<int32_t> point_nobs, edge_point, edge_pose;
    double huber_delta = (double)(float)2.4476519;   // sqrt(5.991) as float
    double chi2_threshold = 5.991;
    // results
    std::vector<uint8_t> edge_status, point_bad;
    orbx_ba_stats stats{};

    orbx_ba_problem view()
    {
        orbx_ba_problem p;
        p.n_poses = (int)pose_fixed.size();
        p.n_points = (int)point_id.size();
        p.n_edges = (int)edge_point.size();
        p.pose_q = pose_q.data();
        p.pose_t = pose_t.data();
        p.pose_fixed = pose_fixed.data();
        p.pose_id = pose_id.data();
        p.pose_cam = pose_cam.data();
        p.points = points.data();
        p.point_id = point_id.data();
        p.point_nobs = point_nobs.data();
        p.edge_point = edge_point.data();
        p.edge_pose = edge_pose.data();
        p.edge_obs = edge_obs.data();
        p.edge_inv_sigma2 = edge_inv_sigma2.data();
        p.huber_delta = huber_delta;
        p.chi2_threshold = chi2_threshold;
        return p;
    }
};

// ---------------------------------------------------------------------------
// Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:154-285): the fields
// of Frame it reads and writes.  mp_xyz holds pMP->GetWorldPos() for the
// keypoints whose mvpMapPoints entry is set (has_mp).
// ---------------------------------------------------------------------------
struct PoseFrame {
    std::vector<KeyPoint> keys_un;          // mvKeysUn
    std::vector<float> inv_level_sigma2;    // mvInvLevelSigma2
    std::vector<uint8_t> has_mp;            // mvpMapPoints[i] != NULL
    std::vector<float> mp_xyz;              // 3 per keypoint
    float fx = 0, fy = 0, cx = 0, cy = 0;
    float Tcw[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // mTcw, row-major
    std::vector<uint8_t> outlier;           // mvbOutlier
    orbx_pose_stats stats{};
};

struct Sim3KeyFrame;   // below, with Sim3Solver
struct Sim3;
struct EssentialGraph;   // below, after Sim3

class Optimizer {
public:
    // int OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, float th2)
    // (src/Optimizer.cc:791-987); defined below Sim3.
    static int OptimizeSim3(orbx_ctx* ctx, const Sim3KeyFrame& kf1, const Sim3KeyFrame& kf2, std::vector<int>& vMatches1,
                            Sim3& S12, float th2);

    // void OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, g2o::Sim3& Scurw,
    //                             KeyFrameAndPose& NonCorrectedSim3, KeyFrameAndPose& CorrectedSim3,
    //                             map<KeyFrame*, set<KeyFrame*>>& LoopConnections)
    // (src/Optimizer.cc:540-789); defined below EssentialGraph.
    static void OptimizeEssentialGraph(orbx_ctx* ctx, EssentialGraph& G);

    // Returns nInitialCorrespondences - nBad, updates F.Tcw and F.outlier.
    static int PoseOptimization(orbx_ctx* ctx, PoseFrame& F)
    {
        const int n = (int)F.keys_un.size();
        std::vector<float> kp(2 * (size_t)n);
        std::vector<int32_t> oct(n);
        for (int i = 0; i < n; i++) {
            kp[2 * i] = F.keys_un[i].x;
            kp[2 * i + 1] = F.keys_un[i].y;
            oct[i] = F.keys_un[i].octave;
        }
        F.outlier.resize(n, 0);
        orbx_pose_frame f;
        f.n = n;
        f.kp_un = kp.data();
        f.octave = oct.data();
        f.inv_level_sigma2 = F.inv_level_sigma2.data();
        f.nlevels = (int)F.inv_level_sigma2.size();
        f.has_mp = F.has_mp.data();
        f.mp_xyz = F.mp_xyz.data();
        f.cam[0] = F.fx;
        f.cam[1] = F.fy;
        f.cam[2] = F.cx;
        f.cam[3] = F.cy;
        for (int k = 0; k < 16; k++) f.Tcw[k] = F.Tcw[k];
        f.outlier = F.outlier.data();
        int inl = 0;
        check(orbx_pose_optimization(ctx, &f, &inl, &F.stats), "Optimizer::PoseOptimization");
        for (int k = 0; k < 16; k++) F.Tcw[k] = f.Tcw[k];
        return inl;
    }

    // pbStopFlag: LocalMapping's mbAbortBA, polled between LM iterations.
    static void LocalBundleAdjustment(orbx_ctx* ctx, LocalBAProblem& prob, bool* pbStopFlag = nullptr)
    {
        orbx_ba_problem p = prob.view();
        prob.edge_status.assign(p.n_edges, 0);
        prob.point_bad.assign(p.n_points, 0);
        check(orbx_lba_solve(ctx, &p, 5, 10, reinterpret_cast<const volatile uint8_t*>(pbStopFlag),
                             prob.edge_status.data(), prob.point_bad.data(), &prob.stats),
              "Optimizer::LocalBundleAdjustment");
    }
};

// ---------------------------------------------------------------------------
// Initializer (src/Initializer.cc:32-221): the constructor's reference
// keypoints, sigma and iterations, and the two model searches Initialize runs
// on two boost::threads (:97-107) as one device call; Initialize goes on with
// `if(RH>0.40)` and ReconstructH / ReconstructF (:113-116) as a second one.
// ---------------------------------------------------------------------------
struct Point3f {
    float x, y, z;
};

class Initializer {
public:
    // Initializer(const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200) (:32-42),
    // with ReferenceFrame.mvKeysUn passed as such.
    Initializer(const std::vector<KeyPoint>& keys1, float sigma = 1.0f, int iterations = 200, orbx_ctx* ctx = nullptr)
        : mvKeys1(keys1), mSigma(sigma), mMaxIterations(iterations), ctx_(ctx)
    {
        if (!ctx_) {
            own_.reset(new Context(1000, 1.2f, 8, 1, 20, 64, 64));
            ctx_ = own_->get();
        }
    }

    // The part of Initialize before the ratio test (:49-110).  rand() is
    // called as the reference's set loop calls it (:80-95): 8 times per
    // iteration through DUtils::Random::RandomInt, and not at all when there
    // are fewer than 8 matches (where the reference would fail).  H and F are
    // 3x3 row-major and keep their content when no iteration scored above 0.
    // Returns RH = SH / (SH + SF).
    float FindModels(const std::vector<KeyPoint>& keys2, const std::vector<int>& vMatches12,
                     std::vector<bool>& vbMatchesInliersH, float& SH, float H[9],
                     std::vector<bool>& vbMatchesInliersF, float& SF, float F[9])
    {
        int N = 0;
        for (int m : vMatches12) N += m >= 0;
        std::vector<int32_t> draws((size_t)mMaxIterations * 8, 0);
        if (N >= 8)
            for (auto& d : draws) d = (int32_t)std::rand();
        std::vector<uint8_t> inH(N > 0 ? N : 1), inF(N > 0 ? N : 1);
        std::vector<int32_t> m12(vMatches12.begin(), vMatches12.end());
        orbx_init_query q;
        std::memset(&q, 0, sizeof(q));
        q.keys1 = mvKeys1.data();
        q.n1 = (int)mvKeys1.size();
        q.keys2 = keys2.data();
        q.n2 = (int)keys2.size();
        q.matches12 = m12.data();
        q.sigma = mSigma;
        q.max_iter = mMaxIterations;
        q.draws = draws.data();
        q.inliers_h = inH.data();
        q.inliers_f = inF.data();
        q.cap = N;
        if ((int)m12.size() != q.n1) throw orbx_error(ORBX_ERR_ARG, "Initializer::FindModels");
        check(orbx_init_models(ctx_, &q), "Initializer::FindModels");
        SH = q.SH;
        SF = q.SF;
        if (q.best_h >= 0) std::memcpy(H, q.H21, sizeof(q.H21));
        if (q.best_f >= 0) std::memcpy(F, q.F21, sizeof(q.F21));
        vbMatchesInliersH.assign(inH.begin(), inH.begin() + N);
        vbMatchesInliersF.assign(inF.begin(), inF.begin() + N);
        mBestH = q.best_h;
        mBestF = q.best_f;
        return q.RH;
    }

    // bool Initialize(const Frame& CurrentFrame, const vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21,
    //                 vector<cv::Point3f>& vP3D, vector<bool>& vbTriangulated) (:44-119), with
    // CurrentFrame.mvKeysUn and the calibration matrix mK (3x3 row-major) passed as such: FindModels, the ratio
    // test, then ReconstructH or ReconstructF with minParallax 1.0 and minTriangulated 50 as one device call.
    // R21 (3x3 row-major) and t21 keep their content when the function returns false.
    bool Initialize(const std::vector<KeyPoint>& keys2, const std::vector<int>& vMatches12, const float K[9],
                    float R21[9], float t21[3], std::vector<Point3f>& vP3D, std::vector<bool>& vbTriangulated)
    {
        mModel = -1;
        mBestHypothesis = -1;
        std::vector<bool> inH, inF;
        float SH = 0.f, SF = 0.f, H[9] = {0}, F[9] = {0};
        const float RH = FindModels(keys2, vMatches12, inH, SH, H, inF, SF, F);
        mModel = RH > 0.40 ? 0 : 1;   // :113
        const std::vector<bool>& in = mModel ? inF : inH;
        std::vector<uint8_t> inliers(in.size() + 1);
        for (size_t i = 0; i < in.size(); i++) inliers[i] = in[i];
        std::vector<int32_t> m12(vMatches12.begin(), vMatches12.end());
        const int n1 = (int)mvKeys1.size();
        const float cam[4] = {K[0], K[4], K[2], K[5]};
        std::vector<float> p3d((size_t)n1 * 3 + 3);
        std::vector<uint8_t> tri((size_t)n1 + 1);
        orbx_reconstruct_query q;
        std::memset(&q, 0, sizeof(q));
        q.keys1 = mvKeys1.data();
        q.n1 = n1;
        q.keys2 = keys2.data();
        q.n2 = (int)keys2.size();
        q.matches12 = m12.data();
        q.inliers = inliers.data();
        q.model = mModel;
        q.M21 = mModel ? F : H;
        q.cam = cam;
        q.sigma = mSigma;
        q.min_parallax = 1.0f;
        q.min_triangulated = 50;
        q.p3d = p3d.data();
        q.triangulated = tri.data();
        q.cap = n1;
        vP3D.assign(n1, Point3f{0.f, 0.f, 0.f});
        vbTriangulated.assign(n1, false);
        // without a winning model of the chosen kind there is nothing to decompose
        if ((mModel ? mBestF : mBestH) < 0) return false;
        check(orbx_init_reconstruct(ctx_, &q), "Initializer::Initialize");
        mBestHypothesis = q.best;
        if (!q.ok) return false;
        std::memcpy(R21, q.R21, sizeof(q.R21));
        std::memcpy(t21, q.t21, sizeof(q.t21));
        for (int i = 0; i < n1; i++) {
            vP3D[i] = Point3f{p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]};
            vbTriangulated[i] = tri[i] != 0;
        }
        return true;
    }

    int mBestH = -1, mBestF = -1;   // winning iterations of the last call (-1: none)
    int mModel = -1;                // 0: ReconstructH, 1: ReconstructF ran in the last Initialize
    int mBestHypothesis = -1;       // its winning motion hypothesis (-1: none)

private:
    std::vector<KeyPoint> mvKeys1;
    float mSigma;
    int mMaxIterations;
    orbx_ctx* ctx_;
    std::unique_ptr<Context> own_;
};

// ---------------------------------------------------------------------------
// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:220-386): what the
// loop reads of a keyframe, and the loop behind the baseline test and
// ComputeF12 (:249-261) as one device call.
// ---------------------------------------------------------------------------
// A keyframe's pose, camera and level tables, copied from the reference's
// getters: GetRotation() / GetTranslation() / GetCameraCenter() as the
// cv::Mat's float data (row-major 3x3, 3, 3), fx, fy, cx, cy and
// GetScaleFactors() / GetVectorScaleSigma2().
struct KeyFrameGeom {
    float Rcw[9], tcw[3], Ow[3], cam[4];
    std::vector<float> scale_factors, level_sigma2;

    KeyFrameGeom(const float* rotation, const float* translation, const float* camera_center, float fx, float fy,
                 float cx, float cy, const std::vector<float>& mvScaleFactors, const std::vector<float>& mvLevelSigma2)
        : scale_factors(mvScaleFactors), level_sigma2(mvLevelSigma2)
    {
        std::memcpy(Rcw, rotation, sizeof(Rcw));
        std::memcpy(tcw, translation, sizeof(tcw));
        std::memcpy(Ow, camera_center, sizeof(Ow));
        cam[0] = fx;
        cam[1] = fy;
        cam[2] = cx;
        cam[3] = cy;
        if (scale_factors.size() != level_sigma2.size()) throw orbx_error(ORBX_ERR_ARG, "KeyFrameGeom");
    }

    // The view the C calls take; valid while this object lives unchanged.
    orbx_kf_geom view() const
    {
        orbx_kf_geom g;
        g.Rcw = Rcw;
        g.tcw = tcw;
        g.Ow = Ow;
        g.cam = cam;
        g.scale_factors = scale_factors.data();
        g.level_sigma2 = level_sigma2.data();
        g.nlevels = (int)scale_factors.size();
        return g;
    }
};

struct NewPoint {
    int idx1, idx2;     // vMatchedIndices[ikp]
    float x3D[3];       // the MapPoint's position (:370)
};

class LocalMapping {
public:
    explicit LocalMapping(orbx_ctx* ctx) : ctx_(ctx) {}

    // The neighbour loop for the neighbours that passed the baseline test:
    // per neighbour the (idx1, idx2, x3D) of every created point in idx1
    // order.  KF1 / KF2s are the keyframes as the vocabulary-node searches
    // read them, F12s the n ComputeF12 results (3x3 row-major each).  The
    // caller creates the MapPoints from the triples (:370-383); the search
    // of each neighbour skips the keypoints that got a point against an
    // earlier one, as the reference's loop does.
    std::vector<std::vector<NewPoint>> CreateNewMapPoints(const orbx_bow_view& KF1, const KeyFrameGeom& geom1,
                                                          const std::vector<orbx_bow_view>& KF2s,
                                                          const std::vector<KeyFrameGeom>& geom2s,
                                                          const std::vector<float>& F12s, bool checkOri = false)
    {
        const int n = (int)KF2s.size(), n1 = KF1.n;
        if ((int)geom2s.size() != n || (int)F12s.size() != 9 * n)
            throw orbx_error(ORBX_ERR_ARG, "LocalMapping::CreateNewMapPoints");
        std::vector<std::vector<NewPoint>> out(n);
        if (n == 0 || n1 <= 0) return out;
        const orbx_kf_geom g1 = geom1.view();
        std::vector<orbx_kf_geom> g2s;
        for (const KeyFrameGeom& g : geom2s) g2s.push_back(g.view());
        std::vector<std::vector<int32_t>> m12(n, std::vector<int32_t>(n1, -1));
        std::vector<std::vector<float>> xyz(n, std::vector<float>((size_t)n1 * 3, 0.f));
        std::vector<std::vector<uint8_t>> status(n, std::vector<uint8_t>(n1, 0));
        std::vector<int32_t*> pm(n);
        std::vector<float*> px(n);
        std::vector<uint8_t*> ps(n);
        for (int k = 0; k < n; k++) {
            pm[k] = m12[k].data();
            px[k] = xyz[k].data();
            ps[k] = status[k].data();
        }
        std::vector<int> n_matches(n, 0), n_created(n, 0);
        check(orbx_create_new_map_points(ctx_, &KF1, &g1, n, KF2s.data(), g2s.data(), F12s.data(), checkOri ? 1 : 0, 1,
                                         pm.data(), n_matches.data(), px.data(), ps.data(), n_created.data(), nullptr),
              "LocalMapping::CreateNewMapPoints");
        for (int k = 0; k < n; k++)
            for (int i = 0; i < n1; i++)
                if (status[k][i] == 1) {
                    NewPoint p;
                    p.idx1 = i;
                    p.idx2 = m12[k][i];
                    std::memcpy(p.x3D, &xyz[k][(size_t)i * 3], sizeof(p.x3D));
                    out[k].push_back(p);
                }
        return out;
    }

private:
    orbx_ctx* ctx_;
};

// ---------------------------------------------------------------------------
// Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc): the RANSAC of
// LoopClosing::ComputeSim3 between its SearchByBoW and SearchBySim3 calls.
// A keyframe is passed as the arrays the solver reads.
// ---------------------------------------------------------------------------
struct Sim3KeyFrame {
    std::vector<KeyPoint> keys;      // mvKeysUn (the octave is read)
    std::vector<float> pos;          // per keypoint x 3: GetWorldPos() of its map point
    std::vector<uint8_t> valid;      // per keypoint: 1 = a map point that is not isBad()
    float Tcw[16];                   // row-major
    float cam[4];                    // fx, fy, cx, cy
    std::vector<float> sigma2;       // mvLevelSigma2
    std::vector<float> invSigma2;    // mvInvLevelSigma2 (OptimizeSim3 reads KF1's); empty: 1.0f / sigma2, as
                                     // ORBextractor fills it
};

class Sim3Solver {
public:
    // Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const vector<MapPoint*>& vpMatched12) (:37-112), with
    // vpMatched12 as the KF2 keypoint index of each matched map point (or < 0) and, optionally, the
    // GetIndexInKeyFrame(pKF1) of pKF1's map points.
    Sim3Solver(const Sim3KeyFrame& kf1, const Sim3KeyFrame& kf2, const std::vector<int>& vMatches12, orbx_ctx* ctx,
               const std::vector<int>* idx1 = nullptr)
        : kf1_(kf1), kf2_(kf2), m12_(vMatches12.begin(), vMatches12.end()), ctx_(ctx)
    {
        if (idx1) idx1_.assign(idx1->begin(), idx1->end());
        mN1 = (int)kf1_.keys.size();
        if ((int)m12_.size() != mN1 || (idx1 && (int)idx1_.size() != mN1) || kf1_.pos.size() != (size_t)mN1 * 3 ||
            kf1_.valid.size() != (size_t)mN1 || kf2_.pos.size() != kf2_.keys.size() * 3 ||
            kf2_.valid.size() != kf2_.keys.size() || kf1_.sigma2.size() != kf2_.sigma2.size())
            throw orbx_error(ORBX_ERR_ARG, "Sim3Solver::Sim3Solver");
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        mRansacMaxIts = maxIterations;
        mnIterations = 0;
    }

    // cv::Mat iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers) (:140-207): T12 as 16
    // floats (row-major), empty where the reference returns cv::Mat().  One device call evaluates the nIterations
    // iterations from 3 * nIterations rand() values drawn here; a return before the chunk's end leaves the draws
    // of the unexecuted iterations consumed.
    std::vector<float> iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        std::vector<int32_t> draws((size_t)(nIterations > 0 ? nIterations : 0) * 3);
        for (auto& d : draws) d = (int32_t)std::rand();
        std::vector<uint8_t> inl(mN1 > 0 ? mN1 : 1, 0);
        orbx_sim3_query q;
        std::memset(&q, 0, sizeof(q));
        q.keys1 = kf1_.keys.data();
        q.n1 = mN1;
        q.keys2 = kf2_.keys.data();
        q.n2 = (int)kf2_.keys.size();
        q.matches12 = m12_.data();
        q.idx1 = idx1_.empty() ? nullptr : idx1_.data();
        q.pos1 = kf1_.pos.data();
        q.valid1 = kf1_.valid.data();
        q.pos2 = kf2_.pos.data();
        q.valid2 = kf2_.valid.data();
        q.T1w = kf1_.Tcw;
        q.T2w = kf2_.Tcw;
        q.cam1 = kf1_.cam;
        q.cam2 = kf2_.cam;
        q.sigma2_1 = kf1_.sigma2.data();
        q.sigma2_2 = kf2_.sigma2.data();
        q.nlevels = (int)kf1_.sigma2.size();
        q.probability = mRansacProb;
        q.min_inliers = mRansacMinInliers;
        q.max_iterations = mRansacMaxIts;
        q.iter_done = mnIterations;
        q.best_inliers = mnBestInliers;
        q.n_iter = nIterations;
        q.draws = draws.data();
        q.inliers = inl.data();
        q.cap = mN1;
        check(orbx_sim3_ransac(ctx_, &q), "Sim3Solver::iterate");
        N = q.N;
        mnIterations += q.iters_run;
        mnBestInliers = q.best_inliers_out;
        if (q.best_iter >= 0) {
            std::memcpy(mBestRotation, q.R12, sizeof(mBestRotation));
            std::memcpy(mBestTranslation, q.t12, sizeof(mBestTranslation));
            mBestScale = q.s12;
        }
        bNoMore = q.no_more != 0;
        nInliers = q.n_inliers;
        vbInliers.assign(inl.begin(), inl.begin() + mN1);
        if (!q.found) return std::vector<float>();
        return std::vector<float>(q.T12, q.T12 + 16);
    }

    // cv::Mat find(vector<bool>& vbInliers12, int& nInliers) (:209-213)
    std::vector<float> find(std::vector<bool>& vbInliers12, int& nInliers)
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }

    const float* GetEstimatedRotation() const { return mBestRotation; }         // 3x3 row-major
    const float* GetEstimatedTranslation() const { return mBestTranslation; }   // 3
    float GetEstimatedScale() const { return mBestScale; }

    int N = 0;                 // correspondences, known after the first iterate
    int mnIterations = 0;
    int mnBestInliers = 0;

private:
    Sim3KeyFrame kf1_, kf2_;
    std::vector<int32_t> m12_, idx1_;
    orbx_ctx* ctx_;
    int mN1 = 0;
    double mRansacProb = 0.99;
    int mRansacMinInliers = 6, mRansacMaxIts = 300;
    float mBestRotation[9] = {0}, mBestTranslation[3] = {0}, mBestScale = 0.f;
};

// ---------------------------------------------------------------------------
// g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3/sim3.h) as a value: the rotation as
// a quaternion (x, y, z, w) that is never renormalised, t and s, and
// Optimizer::OptimizeSim3 (src/Optimizer.cc:791-987), step 4 of
// LoopClosing::ComputeSim3.
// ---------------------------------------------------------------------------
struct Sim3 {
    double q[4] = {0, 0, 0, 1};   // x, y, z, w
    double t[3] = {0, 0, 0};
    double s = 1.0;
    // the floats a Sim3 was built from, kept while it is unchanged: q -> R -> float need not return the bits of a
    // float matrix that is orthonormal to float precision only, and OptimizeSim3 starts from exactly those bits
    float fR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, ft[3] = {0, 0, 0}, fs = 1.f;
    bool from_float = false;

    Sim3() {}
    // g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s): the float values widened, Eigen's
    // Quaterniond(R), no normalisation
    Sim3(const float R[9], const float t_[3], float s_)
    {
        double m[9];
        for (int i = 0; i < 9; i++) m[i] = (double)R[i];
        double tr = m[0] + m[4] + m[8];
        if (tr > 0) {
            tr = std::sqrt(tr + 1.0);
            q[3] = 0.5 * tr;
            tr = 0.5 / tr;
            q[0] = (m[7] - m[5]) * tr;
            q[1] = (m[2] - m[6]) * tr;
            q[2] = (m[3] - m[1]) * tr;
        } else {
            int i = 0;
            if (m[4] > m[0]) i = 1;
            if (m[8] > m[i * 4]) i = 2;
            const int j = (i + 1) % 3, k = (i + 2) % 3;
            tr = std::sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0);
            q[i] = 0.5 * tr;
            tr = 0.5 / tr;
            q[3] = (m[k * 3 + j] - m[j * 3 + k]) * tr;
            q[j] = (m[j * 3 + i] + m[i * 3 + j]) * tr;
            q[k] = (m[k * 3 + i] + m[i * 3 + k]) * tr;
        }
        for (int i = 0; i < 3; i++) t[i] = (double)t_[i];
        s = (double)s_;
        std::memcpy(fR, R, sizeof(fR));
        std::memcpy(ft, t_, sizeof(ft));
        fs = s_;
        from_float = true;
    }

    // Eigen's Quaternion * Vector3
    void rotate(const double v[3], double o[3]) const
    {
        double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
        for (int i = 0; i < 3; i++) uv[i] += uv[i];
        const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
        for (int i = 0; i < 3; i++) o[i] = v[i] + q[3] * uv[i] + c[i];
    }

    // Sim3::operator* (sim3.h:266-272), as in gScm * gSmw (src/LoopClosing.cc:341)
    Sim3 operator*(const Sim3& o) const
    {
        Sim3 r;
        r.q[3] = q[3] * o.q[3] - q[0] * o.q[0] - q[1] * o.q[1] - q[2] * o.q[2];
        r.q[0] = q[3] * o.q[0] + q[0] * o.q[3] + q[1] * o.q[2] - q[2] * o.q[1];
        r.q[1] = q[3] * o.q[1] + q[1] * o.q[3] + q[2] * o.q[0] - q[0] * o.q[2];
        r.q[2] = q[3] * o.q[2] + q[2] * o.q[3] + q[0] * o.q[1] - q[1] * o.q[0];
        double rt[3];
        rotate(o.t, rt);
        for (int i = 0; i < 3; i++) r.t[i] = s * rt[i] + t[i];
        r.s = s * o.s;
        return r;
    }

    // rotation().toRotationMatrix(), translation() and scale() as the floats Converter::toCvMat makes of them
    void to_float(float R[9], float t_[3], float& s_) const
    {
        if (from_float) {
            std::memcpy(R, fR, sizeof(fR));
            std::memcpy(t_, ft, sizeof(ft));
            s_ = fs;
            return;
        }
        const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
        const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
        const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
        const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
        const double m[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz),
                             tyz - twx,       txz - twy, tyz + twx, 1 - (txx + tyy)};
        for (int i = 0; i < 9; i++) R[i] = (float)m[i];
        for (int i = 0; i < 3; i++) t_[i] = (float)t[i];
        s_ = (float)s;
    }
};

// vMatches1: per keypoint of kf1 the KF2 keypoint index of vpMatches1[i] (GetIndexInKeyFrame(pKF2)), -1 for NULL,
// any other negative for a point KF2 does not observe; entries the checks remove become -1.  S12 enters as the
// float matrix, vector and scale ComputeSim3 builds it from (:324-327: the Sim3Solver's estimate) and is replaced
// by the optimised g2oS12 unless the call returns 0 at the nCorrespondences - nBad < 10 exit.  Returns nIn.
inline int Optimizer::OptimizeSim3(orbx_ctx* ctx, const Sim3KeyFrame& kf1, const Sim3KeyFrame& kf2,
                                   std::vector<int>& vMatches1, Sim3& S12, float th2)
{
    const int n1 = (int)kf1.keys.size(), n2 = (int)kf2.keys.size();
    if ((int)vMatches1.size() != n1 || kf1.pos.size() != (size_t)n1 * 3 || kf1.valid.size() != (size_t)n1 ||
        kf2.pos.size() != (size_t)n2 * 3 || kf2.valid.size() != (size_t)n2 || kf1.sigma2.size() != kf2.sigma2.size() ||
        (!kf1.invSigma2.empty() && kf1.invSigma2.size() != kf1.sigma2.size()))
        throw orbx_error(ORBX_ERR_ARG, "Optimizer::OptimizeSim3");
    std::vector<float> inv(kf1.invSigma2);
    if (inv.empty())
        for (float v : kf1.sigma2) inv.push_back(1.0f / v);   // mvInvLevelSigma2[i] = 1.0f / mvLevelSigma2[i]
    std::vector<int32_t> m(vMatches1.begin(), vMatches1.end());
    orbx_sim3_opt_query q;
    std::memset(&q, 0, sizeof(q));
    q.keys1 = kf1.keys.data();
    q.n1 = n1;
    q.keys2 = kf2.keys.data();
    q.n2 = n2;
    q.matches12 = m.data();
    q.pos1 = kf1.pos.data();
    q.valid1 = kf1.valid.data();
    q.pos2 = kf2.pos.data();
    q.valid2 = kf2.valid.data();
    q.T1w = kf1.Tcw;
    q.T2w = kf2.Tcw;
    q.cam1 = kf1.cam;
    q.cam2 = kf2.cam;
    q.inv_sigma2_1 = inv.data();
    q.sigma2_2 = kf2.sigma2.data();   // GetSigma2, as the reference (:912)
    q.nlevels = (int)kf1.sigma2.size();
    S12.to_float(q.R12, q.t12, q.s12);
    q.th2 = th2;
    check(orbx_optimize_sim3(ctx, &q), "Optimizer::OptimizeSim3");
    vMatches1.assign(m.begin(), m.end());
    if (!q.returned_early) {
        for (int i = 0; i < 4; i++) S12.q[i] = q.q12[i];
        for (int i = 0; i < 3; i++) S12.t[i] = q.t12d[i];
        S12.s = q.s12d;
        S12.from_float = false;
    }
    return q.n_in;
}

// ---------------------------------------------------------------------------
// Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:540-789), the call of
// LoopClosing::CorrectLoop after SearchAndFuse.  EssentialGraph holds what
// the reference reads from the map, as plain arrays; BuildEdges() is the edge
// list by the rules of :604-729, free of the device.  The reference iterates
// LoopConnections (a std::map keyed by KeyFrame*) and its std::set<KeyFrame*>
// values in pointer order, which no caller can reproduce; this iterates both
// in the caller's order, so the edges' insertion order -- and with it the last
// bits of the sums -- is the caller's.
// ---------------------------------------------------------------------------
struct EssentialGraph {
    struct KeyFrame {
        unsigned long mnId = 0;
        float Tcw[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};   // GetRotation() row-major, GetTranslation(); out: SetPose
        long long parent = -1;                  // GetParent()->mnId, -1: none
        std::vector<unsigned long> loopEdges;   // GetLoopEdges()
        std::vector<unsigned long> covisibles;  // GetCovisiblesByWeight(100), in its order (bad keyframes are skipped)
        std::vector<unsigned long> children;    // mspChildrens (hasChild)
        bool hasCorrected = false, hasNonCorrected = false;   // CorrectedSim3.count / NonCorrectedSim3.count
        Sim3 corrected, nonCorrected;
    };
    struct Connection {
        unsigned long id;   // the connected keyframe
        int weight;         // pKF->GetWeight(it)
    };
    struct LoopConnection {
        unsigned long id;   // the key of LoopConnections
        std::vector<Connection> to;
    };
    struct MapPoint {
        float pos[3];       // GetWorldPos(); out: SetWorldPos
        long long refKF;    // mnCorrectedReference where mnCorrectedByKF == pCurKF->mnId, else the reference
                            // keyframe's mnId (:765-774); -1: isBad(), left alone
    };
    std::vector<KeyFrame> keyframes;   // pMap->GetAllKeyFrames() without the bad ones
    unsigned long loopKF = 0, curKF = 0;
    std::vector<LoopConnection> loopConnections;
    std::vector<MapPoint> points;
    // out
    std::vector<Sim3> optimised;       // per keyframe: the vertex's estimate
    int iterations = 0, trials = 0, notPosDef = 0;
    double chi2First = 0, chi2Last = 0;

    // index of a keyframe id, -1 when the map holds no such (good) keyframe
    int IndexOf(unsigned long id) const
    {
        for (size_t k = 0; k < keyframes.size(); k++)
            if (keyframes[k].mnId == id) return (int)k;
        return -1;
    }

    // The edges in g2o's insertion order (:604-729).  Throws for a parent, a loop edge or a loop connection that
    // names a keyframe the map does not hold (the reference would dereference a null vertex).
    std::vector<orbx_essgraph_edge> BuildEdges() const
    {
        const int minFeat = 100;
        std::vector<orbx_essgraph_edge> edges;
        std::set<std::pair<unsigned long, unsigned long>> sInsertedEdges;
        auto need = [&](unsigned long id) {
            const int k = IndexOf(id);
            if (k < 0) throw orbx_error(ORBX_ERR_ARG, "EssentialGraph::BuildEdges");
            return k;
        };
        auto has = [](const std::vector<unsigned long>& v, unsigned long id) {
            return std::find(v.begin(), v.end(), id) != v.end();
        };
        // SET LOOP EDGES (:609-637)
        for (const LoopConnection& lc : loopConnections) {
            const int i = need(lc.id);
            for (const Connection& c : lc.to) {
                if ((lc.id != curKF || c.id != loopKF) && c.weight < minFeat) continue;
                edges.push_back({i, need(c.id), 0});
                sInsertedEdges.insert({std::min(lc.id, c.id), std::max(lc.id, c.id)});
            }
        }
        // SET NORMAL EDGES (:640-729)
        for (size_t k = 0; k < keyframes.size(); k++) {
            const KeyFrame& kf = keyframes[k];
            if (kf.parent >= 0) edges.push_back({(int)k, need((unsigned long)kf.parent), 1});   // the spanning tree
            for (unsigned long l : kf.loopEdges)
                if (l < kf.mnId) edges.push_back({(int)k, need(l), 1});
            for (unsigned long n : kf.covisibles) {
                if ((kf.parent >= 0 && n == (unsigned long)kf.parent) || has(kf.children, n) || has(kf.loopEdges, n)) continue;
                const int j = IndexOf(n);
                if (j < 0 || !(n < kf.mnId)) continue;   // isBad(), or the other end adds it
                if (sInsertedEdges.count({std::min(kf.mnId, n), std::max(kf.mnId, n)})) continue;
                edges.push_back({(int)k, j, 1});
            }
        }
        return edges;
    }
};

// Runs the optimisation, then writes the keyframe poses (SetPose) and the map points (SetWorldPos) back into G.
inline void Optimizer::OptimizeEssentialGraph(orbx_ctx* ctx, EssentialGraph& G)
{
    const std::vector<orbx_essgraph_edge> edges = G.BuildEdges();
    const int n = (int)G.keyframes.size(), np = (int)G.points.size();
    std::vector<orbx_essgraph_kf> kfs(n);
    auto put = [](const Sim3& S, double* o) {
        for (int i = 0; i < 4; i++) o[i] = S.q[i];
        for (int i = 0; i < 3; i++) o[4 + i] = S.t[i];
        o[7] = S.s;
    };
    for (int k = 0; k < n; k++) {
        const EssentialGraph::KeyFrame& kf = G.keyframes[k];
        std::memset(&kfs[k], 0, sizeof(kfs[k]));
        kfs[k].id = (int64_t)kf.mnId;
        std::memcpy(kfs[k].Tcw, kf.Tcw, sizeof(kf.Tcw));
        kfs[k].has_corrected = kf.hasCorrected;
        kfs[k].has_noncorrected = kf.hasNonCorrected;
        if (kf.hasCorrected) put(kf.corrected, kfs[k].corrected);
        if (kf.hasNonCorrected) put(kf.nonCorrected, kfs[k].noncorrected);
    }
    std::vector<float> pos(3 * (size_t)np), pos_out(3 * (size_t)np), Tcw(12 * (size_t)n);
    std::vector<int32_t> ref(np);
    std::vector<double> est(8 * (size_t)n);
    for (int k = 0; k < np; k++) {
        std::memcpy(&pos[3 * (size_t)k], G.points[k].pos, 12);
        ref[k] = G.points[k].refKF < 0 ? -1 : G.IndexOf((unsigned long)G.points[k].refKF);
        if (G.points[k].refKF >= 0 && ref[k] < 0) throw orbx_error(ORBX_ERR_ARG, "Optimizer::OptimizeEssentialGraph");
    }
    orbx_essgraph_query q;
    std::memset(&q, 0, sizeof(q));
    q.kfs = kfs.data();
    q.n_kf = n;
    q.loop_kf = G.IndexOf(G.loopKF);
    q.cur_kf = G.IndexOf(G.curKF);
    q.edges = edges.data();
    q.n_edges = (int)edges.size();
    q.pos = pos.data();
    q.ref_kf = ref.data();
    q.n_points = np;
    q.Tcw_out = Tcw.data();
    q.pos_out = pos_out.data();
    q.est_out = est.data();
    check(orbx_optimize_essential_graph(ctx, &q), "Optimizer::OptimizeEssentialGraph");
    G.optimised.assign(n, Sim3());
    for (int k = 0; k < n; k++) {
        std::memcpy(G.keyframes[k].Tcw, &Tcw[12 * (size_t)k], 48);
        for (int i = 0; i < 4; i++) G.optimised[k].q[i] = est[8 * (size_t)k + i];
        for (int i = 0; i < 3; i++) G.optimised[k].t[i] = est[8 * (size_t)k + 4 + i];
        G.optimised[k].s = est[8 * (size_t)k + 7];
    }
    for (int k = 0; k < np; k++)
        if (ref[k] >= 0) std::memcpy(G.points[k].pos, &pos_out[3 * (size_t)k], 12);
    G.iterations = q.iterations;
    G.trials = q.trials;
    G.notPosDef = q.not_posdef;
    G.chi2First = q.chi2_first;
    G.chi2Last = q.chi2_last;
}

// ---------------------------------------------------------------------------
// PnPsolver (include/PnPsolver.h, src/PnPsolver.cc): the RANSAC of
// Tracking::Relocalisation between SearchByBoW and PoseOptimization.  The
// frame is passed as the arrays the solver reads.
// ---------------------------------------------------------------------------
struct PnPFrame {
    std::vector<KeyPoint> keys;      // mvKeysUn (pt and octave are read)
    float cam[4];                    // fx, fy, cx, cy
    std::vector<float> sigma2;       // mvLevelSigma2
};

class PnPsolver {
public:
    // PnPsolver(const Frame& F, const vector<MapPoint*>& vpMapPointMatches) (:39-82), with vpMapPointMatches as
    // GetWorldPos() per keypoint (x 3) and a flag per keypoint (0: NULL or isBad()).
    PnPsolver(const PnPFrame& F, const std::vector<float>& vMapPointPos, const std::vector<uint8_t>& vbMapPoint,
              orbx_ctx* ctx)
        : F_(F), pos_(vMapPointPos), valid_(vbMapPoint), ctx_(ctx)
    {
        mN = (int)F_.keys.size();
        if (pos_.size() != (size_t)mN * 3 || valid_.size() != (size_t)mN) throw orbx_error(ORBX_ERR_ARG, "PnPsolver::PnPsolver");
        mvbBestInliers.assign(mN > 0 ? mN : 1, 0);
        std::memset(mBestTcw, 0, sizeof(mBestTcw));
        SetRansacParameters();
    }

    // SetRansacParameters (:93-129), its arithmetic as written: mRansacMinInliers and mRansacMaxIts are the values
    // adjusted to the number of correspondences, which find() and the loop use.  The device call receives the
    // caller's values and adjusts them in the same way.
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
                             float epsilon = 0.4, float th2 = 5.991)
    {
        mRansacProb = probability;
        mMinInliersArg = minInliers;
        mMaxIterationsArg = maxIterations;
        mRansacMinSet = minSet;
        mEpsilonArg = epsilon;
        mRansacTh = th2;
        N = 0;
        for (uint8_t v : valid_) N += v != 0;
        int nMinInliers = N * epsilon;
        if (nMinInliers < minInliers) nMinInliers = minInliers;
        if (nMinInliers < minSet) nMinInliers = minSet;
        mRansacMinInliers = nMinInliers;
        mRansacMaxIts = 0;   // N < mRansacMinInliers: iterate returns at once (:145-149)
        if (N >= nMinInliers) {
            float eps = epsilon;
            if (eps < (float)nMinInliers / N) eps = (float)nMinInliers / N;
            int nIterations = 1;
            if (nMinInliers != N) {
                const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)eps, 3)));
                nIterations = !(v < 2147483647.0) ? 2147483647 : (v < 1.0 ? 1 : (int)v);
            }
            mRansacMaxIts = std::max(1, std::min(nIterations, maxIterations));
        }
    }

    // cv::Mat iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers) (:137-230): Tcw as 16
    // floats (row-major), empty where the reference returns cv::Mat().  One device call evaluates every iteration
    // the call can run -- max(nIterations, mRansacMaxIts - mnIterations), the loop's condition being an or -- from
    // four rand() values each, all drawn here: a call that returns early leaves the draws of the iterations it did
    // not execute consumed, so the rand() stream runs ahead of the reference's.  The draws array
    // is padded with zeros up to the length orbx_pnp_ransac asks for; the padding is never read.
    std::vector<float> iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        const int can_run = std::max(0, std::max(nIterations, mRansacMaxIts - mnIterations));
        const int n_draws = std::max(can_run, std::max(nIterations, mMaxIterationsArg - mnIterations));
        std::vector<int32_t> draws((size_t)(n_draws > 0 ? n_draws : 0) * 4, 0);
        for (size_t i = 0; i < (size_t)can_run * 4; i++) draws[i] = (int32_t)std::rand();
        std::vector<uint8_t> inl(mN > 0 ? mN : 1, 0);
        orbx_pnp_query q;
        std::memset(&q, 0, sizeof(q));
        q.keys = F_.keys.data();
        q.n = mN;
        q.pos = pos_.data();
        q.valid = valid_.data();
        q.cam = F_.cam;
        q.sigma2 = F_.sigma2.data();
        q.nlevels = (int)F_.sigma2.size();
        q.probability = mRansacProb;
        q.min_inliers = mMinInliersArg;
        q.max_iterations = mMaxIterationsArg;
        q.min_set = mRansacMinSet;
        q.epsilon = mEpsilonArg;
        q.th2 = mRansacTh;
        q.iter_done = mnIterations;
        q.best_inliers = mnBestInliers;
        q.best_mask = mvbBestInliers.data();
        std::memcpy(q.best_Tcw, mBestTcw, sizeof(mBestTcw));
        q.n_iter = nIterations;
        q.n_draws = n_draws;
        q.draws = draws.data();
        q.inliers = inl.data();
        q.cap = mN;
        check(orbx_pnp_ransac(ctx_, &q), "PnPsolver::iterate");
        N = q.N;
        mnIterations = q.iter_done;
        mnBestInliers = q.best_inliers;
        std::memcpy(mBestTcw, q.best_Tcw, sizeof(mBestTcw));
        bNoMore = q.no_more != 0;
        nInliers = q.n_inliers;
        vbInliers.assign(inl.begin(), inl.begin() + mN);
        if (!q.found) {
            vbInliers.clear();
            return std::vector<float>();
        }
        return std::vector<float>(q.Tcw, q.Tcw + 16);
    }

    // cv::Mat find(vector<bool>& vbInliers, int& nInliers) (:131-135): iterate(mRansacMaxIts) with the adjusted value
    std::vector<float> find(std::vector<bool>& vbInliers, int& nInliers)
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
    }

    int N = 0;                 // correspondences
    int mRansacMinInliers = 8, mRansacMaxIts = 0;   // as SetRansacParameters adjusted them
    int mnIterations = 0;
    int mnBestInliers = 0;
    std::vector<uint8_t> mvbBestInliers;   // by keypoint index
    float mBestTcw[16];

private:
    PnPFrame F_;
    std::vector<float> pos_;
    std::vector<uint8_t> valid_;
    orbx_ctx* ctx_;
    int mN = 0;
    double mRansacProb = 0.99;
    int mMinInliersArg = 8, mMaxIterationsArg = 300, mRansacMinSet = 4;   // the caller's arguments
    float mEpsilonArg = 0.4f, mRansacTh = 5.991f;
};

// ---------------------------------------------------------------------------
// KeyFrameDatabase (include/KeyFrameDatabase.h:42-66, src/KeyFrameDatabase.cc)
// in HBM.  Keyframes are named by KeyFrame::mnId (below `capacity`); where the
// reference takes a KeyFrame* or Frame* for its mBowVec, this takes a
// BowVector: the slot the frame is resident in (after orbx_dev_compute_bow) or
// the map's (word, value) pairs in iteration order.
// ---------------------------------------------------------------------------
struct BowVector {
    int slot = -1;
    std::vector<uint32_t> words;
    std::vector<double> values;
    BowVector() = default;
    explicit BowVector(int device_slot) : slot(device_slot) {}
    BowVector(std::vector<uint32_t> w, std::vector<double> v) : words(std::move(w)), values(std::move(v)) {}
};

class KeyFrameDatabase {
public:
    KeyFrameDatabase(orbx_ctx* ctx, int capacity, int maxWords) : ctx_(ctx), capacity_(capacity)
    {
        if (orbx_abi_version() != ORBX_ABI_VERSION) throw orbx_error(ORBX_ERR_UNSUPPORTED, "orbx_abi_version");
        check(orbx_kfdb_create(ctx, capacity, maxWords, &db_), "KeyFrameDatabase");
    }
    ~KeyFrameDatabase() { orbx_kfdb_destroy(db_); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    // void add(KeyFrame* pKF) (:39-45)
    void add(int mnId, const BowVector& bow)
    {
        if (bow.slot >= 0) check(orbx_kfdb_add_slot(ctx_, db_, mnId, bow.slot), "KeyFrameDatabase::add");
        else
            check(orbx_kfdb_add(ctx_, db_, mnId, (int)bow.words.size(), bow.words.data(), bow.values.data()),
                  "KeyFrameDatabase::add");
    }
    // void erase(KeyFrame* pKF) (:47-66)
    void erase(int mnId) { check(orbx_kfdb_erase(ctx_, db_, mnId), "KeyFrameDatabase::erase"); }
    // void clear() (:68-72)
    void clear() { check(orbx_kfdb_clear(ctx_, db_), "KeyFrameDatabase::clear"); }
    int size() const { return orbx_kfdb_size(db_); }

    // Where KeyFrame::UpdateBestCovisibles runs (src/KeyFrame.cc:141-160): what
    // GetBestCovisibilityKeyFrames(10) returns for keyframe mnId from now on.
    void SetBestCovisibles(int mnId, const std::vector<int>& vpOrdered)
    {
        int32_t row[ORBX_KFDB_NEIGHBOURS];
        for (int k = 0; k < ORBX_KFDB_NEIGHBOURS; k++) row[k] = k < (int)vpOrdered.size() ? vpOrdered[k] : -1;
        const int32_t id = mnId;
        check(orbx_kfdb_set_neighbours(ctx_, db_, 1, &id, row), "KeyFrameDatabase::SetBestCovisibles");
    }

    // vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore) (:75-196);
    // spConnectedKeyFrames is pKF->GetConnectedKeyFrames()
    std::vector<int> DetectLoopCandidates(const BowVector& pKF, float minScore,
                                          const std::vector<int>& spConnectedKeyFrames)
    {
        return run(ORBX_KFDB_LOOP, pKF, minScore, std::vector<int>(), spConnectedKeyFrames);
    }
    // LoopClosing::DetectLoop's minScore loop over vpCovisible =
    // GetVectorCovisibleKeyFrames() (src/LoopClosing.cc:122-136) and the call
    // above, in one device call; mMinScore holds the score used.
    std::vector<int> DetectLoopCandidates(const BowVector& pKF, const std::vector<int>& vpCovisible,
                                          const std::vector<int>& spConnectedKeyFrames)
    {
        return run(ORBX_KFDB_LOOP, pKF, 1.0f, vpCovisible, spConnectedKeyFrames);
    }
    // vector<KeyFrame*> DetectRelocalisationCandidates(Frame* F) (:198-308)
    std::vector<int> DetectRelocalisationCandidates(const BowVector& F)
    {
        return run(ORBX_KFDB_RELOC, F, 0.f, std::vector<int>(), std::vector<int>());
    }
    // mpVoc->score(query, keyframe) for the named keyframes
    std::vector<float> score(const BowVector& q, const std::vector<int>& ids)
    {
        std::vector<float> s(ids.size());
        const std::vector<int32_t> i32(ids.begin(), ids.end());
        check(orbx_kfdb_score(ctx_, db_, q.slot >= 0 ? q.slot : -1, (int)q.words.size(), q.words.data(), q.values.data(),
                              (int)ids.size(), i32.data(), s.data()),
              "KeyFrameDatabase::score");
        return s;
    }

    float mMinScore = 0.f;                       // the last loop query's minScore
    int mMaxCommonWords = 0, mnScores = 0;       // the last query's maxCommonWords and nscores

private:
    std::vector<int> run(int mode, const BowVector& b, float minScore, const std::vector<int>& ref,
                         const std::vector<int>& exclude)
    {
        const std::vector<int32_t> r32(ref.begin(), ref.end()), e32(exclude.begin(), exclude.end());
        std::vector<int32_t> cand((size_t)capacity_);
        orbx_kfdb_query_args q{};
        q.mode = mode;
        q.slot = b.slot >= 0 ? b.slot : -1;
        q.n_words = (int)b.words.size();
        q.words = b.words.data();
        q.values = b.values.data();
        q.min_score = minScore;
        q.n_ref = (int)r32.size();
        q.ref = r32.data();
        q.n_exclude = (int)e32.size();
        q.exclude = e32.data();
        q.candidates = cand.data();
        q.cap = capacity_;
        check(orbx_kfdb_query(ctx_, db_, &q), "KeyFrameDatabase::Detect");
        mMinScore = q.min_score_used;
        mMaxCommonWords = q.max_common_words;
        mnScores = q.n_scored;
        return std::vector<int>(cand.begin(), cand.begin() + q.n_candidates);
    }
    orbx_ctx* ctx_;
    orbx_kfdb* db_ = nullptr;
    int capacity_;
};

// ---------------------------------------------------------------------------
// The covisibility graph (KeyFrame::mvpMapPoints, mConnectedKeyFrameWeights,
// mvpOrderedConnectedKeyFrames of every keyframe) in HBM, with the reference's
// method names.  Keyframes and map points are named by mnId; where the
// reference's order depends on KeyFrame* values, the keyframe's `key` stands
// for the pointer: pass (uint64_t)(uintptr_t)pKF to AddKeyFrame.
// ---------------------------------------------------------------------------
class CovisibilityGraph {
public:
    CovisibilityGraph(orbx_ctx* ctx, int kfCapacity, int mpCapacity, int maxKeypoints)
        : ctx_(ctx), kf_capacity_(kfCapacity)
    {
        if (orbx_abi_version() != ORBX_ABI_VERSION) throw orbx_error(ORBX_ERR_UNSUPPORTED, "orbx_abi_version");
        check(orbx_covis_create(ctx, kfCapacity, mpCapacity, maxKeypoints, &m_), "CovisibilityGraph");
    }
    ~CovisibilityGraph() { orbx_covis_destroy(m_); }
    CovisibilityGraph(const CovisibilityGraph&) = delete;
    CovisibilityGraph& operator=(const CovisibilityGraph&) = delete;

    // Where LocalMapping::ProcessNewKeyFrame has added the keyframe's
    // observations (src/LocalMapping.cc:130-160): vpMapPoints is
    // GetMapPointMatches() as mnIds, -1 for NULL.
    void AddKeyFrame(int mnId, uint64_t key, const std::vector<int>& vpMapPoints)
    {
        const std::vector<int32_t> mp(vpMapPoints.begin(), vpMapPoints.end());
        check(orbx_covis_add_keyframe(ctx_, m_, mnId, key, (int)mp.size(), mp.data()), "CovisibilityGraph::AddKeyFrame");
        keys_[mnId] = key;
    }
    // pKF->AddMapPoint(pMP, idx) with pMP->AddObservation(pKF, idx)
    void AddMapPoint(int kfId, int mpId, size_t idx)
    {
        const int32_t i = (int32_t)idx, p = mpId;
        check(orbx_covis_set_matches(ctx_, m_, kfId, 1, &i, &p), "CovisibilityGraph::AddMapPoint");
    }
    // pKF->EraseMapPointMatch(idx) with pMP->EraseObservation(pKF)
    void EraseMapPointMatch(int kfId, size_t idx) { AddMapPoint(kfId, -1, idx); }
    // MapPoint::SetBadFlag of every id (and the old point of MapPoint::Replace)
    void EraseMapPoints(const std::vector<int>& ids)
    {
        const std::vector<int32_t> p(ids.begin(), ids.end());
        check(orbx_covis_erase_points(ctx_, m_, (int)p.size(), p.data()), "CovisibilityGraph::EraseMapPoints");
    }
    // the connection part of KeyFrame::SetBadFlag (src/KeyFrame.cc:510-521)
    void EraseKeyFrame(int mnId) { check(orbx_covis_erase_keyframe(ctx_, m_, mnId), "CovisibilityGraph::EraseKeyFrame"); }
    int size() const { return orbx_covis_size(m_); }

    // void KeyFrame::UpdateConnections() (:332-421).  Returns false where the
    // reference returns at `if(KFcounter.empty())`; mFront is then -1, else
    // mvpOrderedConnectedKeyFrames.front() (mpParent under mbFirstConnection).
    bool UpdateConnections(int mnId, int th = 15)
    {
        const int32_t id = mnId;
        int32_t updated = 0, front = -1;
        check(orbx_covis_update_connections(ctx_, m_, 1, &id, th, &updated, &front), "CovisibilityGraph::UpdateConnections");
        mFront = front;
        return updated != 0;
    }
    // CorrectLoop's loop over the connected keyframes (src/LoopClosing.cc:
    // 411-412), in the given order; fronts as above.
    std::vector<int> UpdateConnections(const std::vector<int>& ids, int th = 15)
    {
        const std::vector<int32_t> i32(ids.begin(), ids.end());
        std::vector<int32_t> updated(ids.size() + 1), front(ids.size() + 1);
        check(orbx_covis_update_connections(ctx_, m_, (int)i32.size(), i32.data(), th, updated.data(), front.data()),
              "CovisibilityGraph::UpdateConnections");
        return std::vector<int>(front.begin(), front.begin() + ids.size());
    }

    // vector<KeyFrame*> GetVectorCovisibleKeyFrames() (:171-175); mvOrderedWeights of the call in mWeights
    std::vector<int> GetVectorCovisibleKeyFrames(int mnId) { return read(mnId, ORBX_COVIS_ORDERED); }
    // vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int &N) (:177-185)
    std::vector<int> GetBestCovisibilityKeyFrames(int mnId, int N)
    {
        std::vector<int> v = read(mnId, ORBX_COVIS_ORDERED);
        if ((int)v.size() > N) v.resize((size_t)N);
        return v;
    }
    // set<KeyFrame*> GetConnectedKeyFrames() (:162-169), in the set's order
    std::vector<int> GetConnectedKeyFrames(int mnId) { return read(mnId, ORBX_COVIS_ALL); }
    // int GetWeight(KeyFrame* pKF) (:204-211)
    int GetWeight(int mnId, int pKF)
    {
        const std::vector<int> all = read(mnId, ORBX_COVIS_ALL);
        for (size_t k = 0; k < all.size(); k++)
            if (all[k] == pKF) return mWeights[k];
        return 0;
    }
    // vector<KeyFrame*> GetCovisiblesByWeight(const int &w) (:187-202), the
    // reference's upper_bound as it stands: with weightComp(a, b) = a > b it
    // finds the first weight below w, and when every weight is >= w it
    // returns end() and the function an empty vector.
    std::vector<int> GetCovisiblesByWeight(int mnId, int w)
    {
        const std::vector<int> ordered = read(mnId, ORBX_COVIS_ORDERED);
        if (ordered.empty()) return std::vector<int>();
        const std::vector<int>::iterator it =
            std::upper_bound(mWeights.begin(), mWeights.end(), w, [](int a, int b) { return a > b; });
        if (it == mWeights.end()) return std::vector<int>();
        return std::vector<int>(ordered.begin(), ordered.begin() + (it - mWeights.begin()));
    }

    // Tracking::UpdateReference's two functions (src/Tracking.cc:764-865) for
    // mCurrentFrame.mvpMapPoints as mnIds (-1 for NULL).
    struct Reference {
        std::vector<int> mvpLocalKeyFrames, mvpLocalMapPoints;
        int mpReferenceKF = -1;            // pKFmax, -1 for NULL
        int nVoters = 0;                   // keyframes that observe a point of the frame
        std::vector<uint8_t> vbErased;     // 1: the frame's point is bad, NULL it (:805-808)
    };
    Reference UpdateReference(const std::vector<int>& vpMapPoints)
    {
        const std::vector<int32_t> f(vpMapPoints.begin(), vpMapPoints.end());
        Reference r;
        r.vbErased.assign(f.size() + 1, 0);
        std::vector<int32_t> lk((size_t)kf_capacity_), lm(1024);
        orbx_covis_reference_args q{};
        q.n = (int)f.size();
        q.frame_mp = f.data();
        q.frame_erased = r.vbErased.data();
        q.local_kf = lk.data();
        q.kf_cap = kf_capacity_;
        for (;;) {   // the list of points grows with the map: once more with the size the call reported
            q.local_mp = lm.data();
            q.mp_cap = (int)lm.size();
            const int code = orbx_covis_update_reference(ctx_, m_, &q);
            if (code == ORBX_ERR_CAPACITY && q.n_local_mp > q.mp_cap) {
                lm.resize((size_t)q.n_local_mp);
                continue;
            }
            check(code, "CovisibilityGraph::UpdateReference");
            break;
        }
        r.vbErased.resize(f.size());
        r.mvpLocalKeyFrames.assign(lk.begin(), lk.begin() + q.n_local_kf);
        r.mvpLocalMapPoints.assign(lm.begin(), lm.begin() + q.n_local_mp);
        r.mpReferenceKF = q.ref_kf;
        r.nVoters = q.n_voters;
        return r;
    }

    // Where KeyFrame::UpdateBestCovisibles runs: the keyframe's first 10 go to
    // the device KeyFrameDatabase, which accumulates scores over them.
    void PushBestCovisibles(KeyFrameDatabase& db, int mnId)
    {
        db.SetBestCovisibles(mnId, GetBestCovisibilityKeyFrames(mnId, ORBX_KFDB_NEIGHBOURS));
    }

    // mvKeysUn[i].octave of keyframe mnId, one per entry of its row: what
    // KeyFrameCulling reads through GetKeyPointUn(i).octave
    void SetOctaves(int mnId, const std::vector<int>& vOctaves)
    {
        const std::vector<uint8_t> o(vOctaves.begin(), vOctaves.end());
        check(orbx_covis_set_octaves(ctx_, m_, mnId, (int)o.size(), o.data()), "CovisibilityGraph::SetOctaves");
    }

    // The spanning tree (KeyFrame::mpParent, mspChildrens) stays on the host;
    // the children of a keyframe are iterated in key order (a set<KeyFrame*>).
    void ChangeParent(int mnId, int pKF)
    {
        EraseChild(GetParent(mnId), mnId);
        mpParent_[mnId] = pKF;
        if (pKF >= 0) mspChildrens_[pKF].push_back(mnId);
    }
    int GetParent(int mnId) const
    {
        const std::map<int, int>::const_iterator it = mpParent_.find(mnId);
        return it == mpParent_.end() ? -1 : it->second;
    }
    std::vector<int> GetChilds(int mnId) const
    {
        const std::map<int, std::vector<int>>::const_iterator it = mspChildrens_.find(mnId);
        std::vector<int> c = it == mspChildrens_.end() ? std::vector<int>() : it->second;
        std::sort(c.begin(), c.end(), [this](int a, int b) { return keys_.at(a) < keys_.at(b); });
        return c;
    }

    // void LocalMapping::KeyFrameCulling() (src/LocalMapping.cc:539-593) for
    // mpCurrentKeyFrame; vpNotErase: the keyframes whose mbNotErase is set
    // (LoopClosing holds them).  The walk, the connection part of every
    // SetBadFlag and its EraseObservations run on the device, one cull per
    // call: after each, the tree part of SetBadFlag (src/KeyFrame.cc:523-581)
    // runs here on the children's lists as that cull left them, and the call
    // resumes with the rest of the list.
    struct Culling {
        std::vector<int> vpCulled;        // SetBadFlag ran: mpMap->EraseKeyFrame, mpKeyFrameDB->erase are the caller's
        std::vector<int> vpToBeErased;    // redundant, but mbNotErase: mbToBeErased = true
        std::vector<int> vpBadMapPoints;  // MapPoint::SetBadFlag ran through EraseObservation
    };
    Culling KeyFrameCulling(int mpCurrentKeyFrame, const std::vector<int>& vpNotErase = std::vector<int>())
    {
        Culling out;
        const std::vector<int32_t> keep(vpNotErase.begin(), vpNotErase.end());
        std::vector<int32_t> cand((size_t)kf_capacity_), mps((size_t)kf_capacity_), red((size_t)kf_capacity_),
            dec((size_t)kf_capacity_), bad(256);
        int cur = mpCurrentKeyFrame, first = 0, n_rest = 0;   // the list is cand[first, first + n_rest) once it is known
        for (;;) {
            orbx_covis_cull_args q{};
            q.cur = cur;
            q.n_keep = (int)keep.size();
            q.keep = keep.data();
            q.max_culls = 1;
            q.cand = cand.data() + first;
            q.n_cand = n_rest;
            q.cand_cap = kf_capacity_ - first;
            q.n_mps = mps.data();
            q.n_redundant = red.data();
            q.decision = dec.data();
            q.bad_points = bad.data();
            q.bad_cap = (int)bad.size();
            const int code = orbx_covis_cull_keyframes(ctx_, m_, &q);
            if (code == ORBX_ERR_CAPACITY && q.n_bad > q.bad_cap) {   // nothing changed: once more with room
                bad.resize((size_t)q.n_bad);
                continue;
            }
            check(code, "CovisibilityGraph::KeyFrameCulling");
            out.vpBadMapPoints.insert(out.vpBadMapPoints.end(), bad.begin(), bad.begin() + q.n_bad);
            for (int k = 0; k < q.n_done; k++) {
                const int pKF = cand[(size_t)(first + k)];
                if (dec[(size_t)k] == 2) out.vpToBeErased.push_back(pKF);
                if (dec[(size_t)k] != 1) continue;
                out.vpCulled.push_back(pKF);
                UpdateSpanningTree(pKF);
            }
            if (q.n_done >= q.n_cand) break;
            cur = -1;
            first += q.n_done;
            n_rest = q.n_cand - q.n_done;
        }
        return out;
    }

    // void LocalMapping::MapPointCulling() (src/LocalMapping.cc:190-218): the
    // list loses what the reference erases from it; returns the points whose
    // SetBadFlag ran.
    struct RecentMapPoint {
        int mnId, mnFound, mnVisible, mnFirstKFid;
    };
    std::vector<int> MapPointCulling(int nCurrentKFid, std::list<RecentMapPoint>& mlpRecentAddedMapPoints)
    {
        std::vector<int32_t> ids, found, visible, first;
        for (const RecentMapPoint& p : mlpRecentAddedMapPoints) {
            ids.push_back(p.mnId);
            found.push_back(p.mnFound);
            visible.push_back(p.mnVisible);
            first.push_back(p.mnFirstKFid);
        }
        std::vector<int32_t> action(ids.size() + 1);
        check(orbx_covis_cull_points(ctx_, m_, nCurrentKFid, (int)ids.size(), ids.data(), found.data(), visible.data(),
                                     first.data(), action.data()),
              "CovisibilityGraph::MapPointCulling");
        std::vector<int> vpBad;
        size_t k = 0;
        for (std::list<RecentMapPoint>::iterator lit = mlpRecentAddedMapPoints.begin();
             lit != mlpRecentAddedMapPoints.end(); k++) {
            if (action[k] == 2 || action[k] == 3) vpBad.push_back(lit->mnId);
            if (action[k] != 0) lit = mlpRecentAddedMapPoints.erase(lit);
            else lit++;
        }
        return vpBad;
    }

    int mFront = -1;              // the last single UpdateConnections' front
    std::vector<int> mWeights;    // the weights of the last read, entry for entry

private:
    void EraseChild(int pKF, int child)
    {
        if (pKF < 0) return;
        std::vector<int>& c = mspChildrens_[pKF];
        c.erase(std::remove(c.begin(), c.end(), child), c.end());
    }
    // "Update Spanning Tree" of KeyFrame::SetBadFlag (src/KeyFrame.cc:523-581)
    // for a keyframe the device has just culled: its children are erased
    // members' entries no more, and the lists are read as they stand now.
    void UpdateSpanningTree(int mnId)
    {
        const int mpParent = GetParent(mnId);
        if (mpParent < 0) return;   // the caller keeps no tree here
        std::vector<int> sParentCandidates(1, mpParent);
        std::vector<int> mspChildrens = GetChilds(mnId);
        while (!mspChildrens.empty()) {
            bool bContinue = false;
            int max = -1, pC = -1, pP = -1;
            for (int pKF : mspChildrens) {
                const std::vector<int> vpConnected = GetVectorCovisibleKeyFrames(pKF);
                for (size_t i = 0; i < vpConnected.size(); i++)
                    for (int cand : sParentCandidates)
                        if (vpConnected[i] == cand) {
                            const int w = mWeights[i];   // GetWeight(vpConnected[i])
                            if (w > max) {
                                pC = pKF;
                                pP = vpConnected[i];
                                max = w;
                                bContinue = true;
                            }
                        }
            }
            if (!bContinue) break;
            ChangeParent(pC, pP);
            sParentCandidates.push_back(pC);
            mspChildrens.erase(std::remove(mspChildrens.begin(), mspChildrens.end(), pC), mspChildrens.end());
        }
        for (int pKF : mspChildrens) ChangeParent(pKF, mpParent);
        EraseChild(mpParent, mnId);
        mpParent_.erase(mnId);
        mspChildrens_.erase(mnId);
    }
    std::map<int, uint64_t> keys_;                   // the KeyFrame* stand-ins, for the order of a set<KeyFrame*>
    std::map<int, int> mpParent_;
    std::map<int, std::vector<int>> mspChildrens_;
    std::vector<int> read(int mnId, int which)
    {
        std::vector<int32_t> kfs((size_t)kf_capacity_), ws((size_t)kf_capacity_);
        int n = 0;
        check(orbx_covis_connections(ctx_, m_, mnId, which, kfs.data(), ws.data(), kf_capacity_, &n),
              "CovisibilityGraph::read");
        mWeights.assign(ws.begin(), ws.begin() + n);
        return std::vector<int>(kfs.begin(), kfs.begin() + n);
    }
    orbx_ctx* ctx_;
    orbx_covis* m_ = nullptr;
    int kf_capacity_;
};

}  // namespace ORB_SLAM_AMD
