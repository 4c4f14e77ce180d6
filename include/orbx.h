/*
 * orbx.h -- C ABI of the MI355X-native ORB-SLAM front end + local-BA kernels.
 *
 * Every entry point below replaces one reference interface on the hot path
 * named by BASELINE.json's north_star.  The reference is
 * a single C++ executable with no FFI layer, so the "binding" is a C++ adapter
 * (orb_slam_amd/adapters/, shown in INTEGRATION.md) that keeps the reference
 * class signatures and calls these functions.  Signatures use plain pointers
 * and sizes only; all device memory is owned by an orbx_ctx.
 *
 * Conventions
 *   - return 0 (ORBX_OK) on success, a negative ORBX_ERR_* code otherwise.
 *     The reference has no error codes (it asserts or returns silently); the
 *     adapter maps codes back to that behaviour.
 *   - host pointers are caller-allocated; "cap" arguments bound outputs.
 *   - an orbx_ctx owns one HIP stream and its buffers; it is NOT thread-safe
 *     (mirrors ORBextractor, whose pyramid is member state:
 *     include/ORBextractor.h:74).  Use one context per calling thread.
 */
#ifndef ORBX_H
#define ORBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI revision of this header.  A caller compares orbx_abi_version() with the
 * ORBX_ABI_VERSION it was compiled against before its first call (the C++
 * adapter does, in every constructor) and refuses a library of another
 * revision instead of calling through a changed signature.
 *   1: rounds 1-3.
 *   2: orbx_lba_solve_batch / orbx_lba_run take per-problem abort flags
 *      (the `aborts` argument after iters1).
 *   3: single-frame graph path (orbx_set_launch_mode), host-fed pipeline
 *      (orbx_host_alloc, orbx_dev_upload_async, orbx_dev_download_async),
 *      image bounds of device-resident frames (orbx_dev_set_image_bounds),
 *      multi-workgroup single local-BA problems (orbx_lba_set_workgroups);
 *      additions only.
 *   4: orbx_pose_set_exact / orbx_pose_get_exact; additions only.
 *   5: the measured-slower opt-in modes removed (orbx_dev_set_pyramid_mode,
 *      orbx_dev_pyramid_fused / _kind, orbx_dev_set_fast_chunk / get, launch
 *      modes 2 and 3); orbx_lba_last_workgroups, orbx_debug_lba_split;
 *      orbx_track_frame (one Tracking frame on the device); PoseOptimization
 *      sums sequentially in g2o's order by default (orbx_pose_set_exact).
 *   6: initialisation models (orbx_init_models, orbx_init_models_batch,
 *      orbx_dev_init_models, orbx_dev_read_init_models); additions only.
 *   7: new map points (orbx_kf_geom, orbx_triangulate_matches,
 *      orbx_create_new_map_points, orbx_dev_create_new_map_points);
 *      additions only.
 *   8: the end of map initialisation (orbx_reconstruct_query,
 *      orbx_init_reconstruct, orbx_init_reconstruct_batch,
 *      orbx_dev_init_reconstruct, orbx_dev_read_init_reconstruct);
 *      additions only.
 *   9: the Sim3 solver of loop closing (orbx_sim3_query, orbx_sim3_ransac,
 *      orbx_sim3_ransac_batch, orbx_sim3_kf, orbx_dev_sim3_candidates);
 *      additions only.
 *  10: the PnP solver of relocalisation (orbx_pnp_query, orbx_pnp_ransac,
 *      orbx_pnp_ransac_batch, orbx_dev_pnp_candidates); additions only.
 *  11: the Sim3 optimisation of loop closing (orbx_sim3_opt_query,
 *      orbx_optimize_sim3, orbx_optimize_sim3_batch, orbx_dev_optimize_sim3);
 *      additions only.
 *  12: the keyframe database in HBM (orbx_kfdb_create / destroy / clear /
 *      size, orbx_kfdb_add, orbx_kfdb_add_slot, orbx_kfdb_erase,
 *      orbx_kfdb_set_neighbours, orbx_kfdb_query, orbx_kfdb_score);
 *      additions only.
 *  13: the essential-graph optimisation of CorrectLoop (orbx_essgraph_kf,
 *      orbx_essgraph_edge, orbx_essgraph_query, orbx_essgraph_plan,
 *      orbx_optimize_essential_graph); additions only.
 *  14: the covisibility graph in HBM (orbx_covis_create / destroy / clear /
 *      size, orbx_covis_add_keyframe, orbx_covis_set_matches,
 *      orbx_covis_erase_points, orbx_covis_erase_keyframe,
 *      orbx_covis_update_connections, orbx_covis_connections,
 *      orbx_covis_update_reference); additions only.
 *  15: LocalMapping's culling on the covisibility graph
 *      (orbx_covis_set_octaves, orbx_covis_cull_keyframes,
 *      orbx_covis_cull_points); additions only. */
#define ORBX_ABI_VERSION 15
int orbx_abi_version(void);

#define ORBX_OK               0
#define ORBX_ERR_ARG         -1  /* invalid argument / shape                      */
#define ORBX_ERR_HIP         -2  /* HIP runtime failure (device missing, launch)  */
#define ORBX_ERR_CAPACITY    -3  /* caller buffer or context capacity too small   */
#define ORBX_ERR_UNSUPPORTED -4  /* configuration outside the implemented subset  */
#define ORBX_ERR_NOMEM       -5  /* device or host allocation failed              */
#define ORBX_ERR_NOT_POSDEF  -6  /* reduced camera system not positive definite   */

/* cv::KeyPoint layout (OpenCV 2.4 core/types.hpp): 28 bytes. */
typedef struct {
    float x, y;        /* pt                                 */
    float size;        /* diameter of the meaningful region  */
    float angle;       /* degrees in [0,360)                 */
    float response;    /* FAST score                         */
    int32_t octave;    /* pyramid level                      */
    int32_t class_id;  /* always -1                          */
} orbx_keypoint;

typedef struct orbx_ctx orbx_ctx;

/* ------------------------------------------------------------------------ */
/* Context / extractor construction                                          */
/* ------------------------------------------------------------------------ */

/* Replaces ORBextractor::ORBextractor(int nfeatures, float scaleFactor,
 * int nlevels, int scoreType, int fastTh)  (src/ORBextractor.cc:457-511,
 * include/ORBextractor.h:37).  max_w/max_h/max_batch size the device
 * buffers (frames larger than max_w x max_h are rejected); max_batch is the
 * number of frames one batched launch may carry and also the number of
 * device-resident frame slots available to orbx_dev_* (see below).
 * score_type: 0 = ORB::HARRIS_SCORE (HarrisResponses re-scores the FAST
 * corners before retainBest, src/ORBextractor.cc:79-120, :616-620; keypoint
 * responses are the Harris values), any other value = FAST_SCORE (the FAST
 * score; the reference tests only == HARRIS_SCORE). */
int  orbx_create(orbx_ctx** out, int device, int nfeatures, float scale_factor,
                 int nlevels, int score_type, int fast_th,
                 int max_w, int max_h, int max_batch);
void orbx_destroy(orbx_ctx* ctx);

/* ORBextractor::GetLevels / GetScaleFactor (include/ORBextractor.h:47-51). */
int   orbx_get_levels(const orbx_ctx* ctx);
float orbx_get_scale_factor(const orbx_ctx* ctx);
/* mnFeaturesPerLevel (src/ORBextractor.cc:476-487) and mvScaleFactor. */
int   orbx_get_features_per_level(const orbx_ctx* ctx, int32_t* out, int cap);
int   orbx_get_scale_factors(const orbx_ctx* ctx, float* out, int cap);

/* Host-side extractor tables for a frame size, computed without a device:
 * per level 8 ints {w, h, n_desired, level_cols, level_rows, nfeatures_cell,
 * n_cells, n_valid_cells} (src/ORBextractor.cc:462-487, 527-547, 786).
 * Returns the number of levels or a negative error. */
int orbx_describe_levels(int nfeatures, float scale_factor, int nlevels, int fast_th,
                         int w, int h, int32_t* out, int cap);

/* ------------------------------------------------------------------------ */
/* A. Extraction                                                             */
/* ------------------------------------------------------------------------ */

/* Replaces ORBextractor::operator()(image, mask=Mat(), keypoints, descriptors)
 * (src/ORBextractor.cc:718-779).  img: w x h mono8 with row stride `stride`.
 * Outputs keypoints in reference order (level-major, retainBest order within
 * a level; coordinates scaled to level 0) and N x 32 descriptor bytes.
 * An empty image (w==0 || h==0) returns ORBX_OK with *n_out = 0 -- the
 * reference returns without touching its outputs (:721-722). */
int orbx_extract(orbx_ctx* ctx, const uint8_t* img, int w, int h, size_t stride,
                 orbx_keypoint* kps, uint8_t* desc, int cap, int* n_out);
/* How orbx_extract issues its work (Frame::Frame calls the extractor once per
 * frame, synchronously: src/Frame.cc:59, src/Tracking.cc:206).
 *   1 (default): the call is one hipGraph launch -- the image copied through a
 *     page-locked staging buffer into its slot, the extraction kernels (the
 *     blur on a branch beside FAST and retainBest), then one kernel that
 *     stores the count, error flags, keypoints and descriptors into a
 *     page-locked buffer -- and one synchronisation.  The graph is captured
 *     on the first call of a configuration (frame size, fp-contract mode,
 *     nth_element era) and replayed after that.
 *   0: the kernels launched one by one on the context stream, with pageable
 *     copies (rounds 1-4).
 * Both produce identical outputs; kernel timing (orbx_dev_kernel_time_enable)
 * takes the stream launches.  (Modes 2 -- the pyramid reading the staging
 * buffer in place -- and 3 -- the single-frame launches without a graph --
 * measured within noise of 1 and were removed in ABI 5.) */
int orbx_set_launch_mode(orbx_ctx* ctx, int mode);
int orbx_get_launch_mode(const orbx_ctx* ctx);

/* Batched form: B frames of identical size, host in / host out.
 * kps: B*cap records, desc: B*cap*32 bytes, n_out: B counts. */
int orbx_extract_batch(orbx_ctx* ctx, int B, const uint8_t* const* imgs,
                       int w, int h, size_t stride,
                       orbx_keypoint* kps, uint8_t* desc, int cap, int32_t* n_out);

/* ------------------------------------------------------------------------ */
/* Device-resident pipeline (inputs already in HBM; used by bench/tests).     */
/* A context owns `max_batch` frame slots.  Frames are uploaded once, then    */
/* extracted and matched without host round-trips.                            */
/* ------------------------------------------------------------------------ */

/* Copy `count` host frames (w x h, contiguous rows of `stride` bytes, frame k
 * at imgs + k*h*stride) into slots [first, first+count).  All slots of one
 * context share one frame size (set by the first upload). */
int orbx_dev_upload(orbx_ctx* ctx, int first, int count, const uint8_t* imgs,
                    int w, int h, size_t stride);
/* Extract slots [first, first+count) (async, on the context stream).
 * Batches of 32+ frames run as two halves on two internal streams (joined
 * before the call's later work) unless disabled with orbx_dev_set_split. */
int orbx_dev_extract(orbx_ctx* ctx, int first, int count);
/* Floating-point evaluation of the expressions that live in the reference's
 * own source rather than in OpenCV: computeOrbDescriptor's sample coordinates
 * x*b + y*a, x*a - y*b (src/ORBextractor.cc:165-167) and HarrisResponses'
 * response (:117-118).  0 (default): each operation rounded as written (ISO
 * C++, the reference built with -ffp-contract=off or on a host without FMA).
 * 1: as GCC evaluates them when it builds the reference with its own flags
 * (-O3 -march=native, CMakeLists.txt:12-13) on an FMA host, where GCC's
 * default -ffp-contract=fast fuses them: fma(x, b, y*a), fma(x, a, -(y*b));
 * fma(-(k*(a+b)), a+b, fma(a, b, -(c*c))).  Applies to extractions launched
 * after the call (DESIGN.md section 4 has the measured effect).
 * The triangulation gates (orbx_triangulate_matches and the two
 * create_new_map_points forms) follow the mode too, for the two expressions
 * of src/LocalMapping.cc:335-351 that are the reference's own source:
 * fx*x*invz+cx and errX*errX+errY*errY as written (0), or fma(fx*x, invz, cx)
 * and fma(errX, errX, errY*errY) (1); they read the mode at the call. */
int orbx_set_fp_contract(orbx_ctx* ctx, int enable);
int orbx_get_fp_contract(const orbx_ctx* ctx);
/* libstdc++ era of retainBest's std::nth_element (KeyPointsFilter::retainBest,
 * called at src/ORBextractor.cc:683, :699).  The surviving keypoints and their
 * order are nth_element's permutation, and libstdc++ changed its introselect
 * pivot step in GCC 4.9 (PR libstdc++/58437):
 *   ORBX_NTH_PIVOT_GCC49 (0): median of (first + 1, mid, last - 1) swapped
 *     into first -- GCC >= 4.9;
 *   ORBX_NTH_PIVOT_GCC48 (1, default): median of (first, mid, last - 1)
 *     moved to first -- GCC 4.6 .. 4.8, the compilers of the platforms the
 *     reference documents (Ubuntu 12.04 / 14.04, README.md:46), whose OpenCV
 *     2.4 packages instantiate retainBest's nth_element.
 * Applies to extractions launched after the call (DESIGN.md section 4 has the
 * measured effect). */
enum { ORBX_NTH_PIVOT_GCC49 = 0, ORBX_NTH_PIVOT_GCC48 = 1 };
int orbx_set_nth_pivot(orbx_ctx* ctx, int mode);
int orbx_get_nth_pivot(const orbx_ctx* ctx);
/* enable: 0 = one stream; 1 = split with the default three parts;
 * 2..4 = split, and the asynchronous extract_match pipeline runs its batch
 * in that many parts on as many streams, part i released by part i-1's
 * FAST pass. */
int orbx_dev_set_split(orbx_ctx* ctx, int enable);
/* orbx_dev_extract followed by matching every slot of the batch against its
 * predecessor (mode 1: orbx_dev_match_prev with window / nnratio / check_ori;
 * mode 2: orbx_dev_match_bf_prev with th_low / nnratio), pipelined: with the
 * two-stream split each half's internal pairs are matched while the other
 * half is still being extracted.  Results as for the separate calls. */
int orbx_dev_extract_match(orbx_ctx* ctx, int first, int count, int seq_len, int mode,
                           int window, int th_low, float nnratio, int check_ori);
/* Asynchronous matching for orbx_dev_extract_match: the batch's matching is
 * queued on an internal stream after its extraction, and the call returns;
 * a later extract_match of *other* slots overlaps it (a stream of batches
 * alternating between two slot ranges keeps extraction and matching of
 * consecutive batches concurrent).  Any other call on the context, or an
 * extraction into slots the pending match reads, waits for it first. */
int orbx_dev_set_async_match(orbx_ctx* ctx, int enable);
/* (ABI 5 removed the opt-in pyramid modes -- one fused pyramid + blur
 * launch per batch, and the band-cascade raw pyramid for batches -- and
 * chunked FAST workgroups: each measured slower than the default at every
 * frame size.  The band cascade remains the pyramid of
 * orbx_extract's single-frame graph, where it is the fastest.) */
/* SearchForInitialization (B3) for slots [first, first+count): slot s is
 * matched against slot s-1 unless s % seq_len == 0 (sequence start).  Frame
 * s-1 plays F1 (initial frame), s plays F2; vbPrevMatched = F1 keypoints. */
int orbx_dev_match_prev(orbx_ctx* ctx, int first, int count, int seq_len,
                        int window, float nnratio, int check_ori);
/* Image bounds of the slots' keypoints for the device-resident matchers
 * (orbx_dev_match_prev and the extract_match pipeline): Frame's static
 * mnMinX, mnMaxX, mnMinY, mnMaxY (src/Frame.cc:320-348), which also scale its
 * 64x48 grid (:76-77).  After orbx_dev_undistort with a distorting camera,
 * pass orbx_compute_image_bounds' result; NULL (the default) is 0..w x 0..h,
 * the reference's bounds without distortion (:341-347). */
int orbx_dev_set_image_bounds(orbx_ctx* ctx, const float* bounds);
/* Brute-force matching (config C3) of slots [first, first+count) against
 * their predecessors, same slot pairing as orbx_dev_match_prev: every
 * keypoint of s-1 against every keypoint of s, accepted when best <= th_low
 * and best < nnratio * second (rule of src/ORBmatcher.cc:640-654); results
 * via orbx_dev_read_matches. */
int orbx_dev_match_bf_prev(orbx_ctx* ctx, int first, int count, int seq_len,
                           int th_low, float nnratio);
int orbx_dev_sync(orbx_ctx* ctx);
/* Host-fed pipeline: frames that arrive in host memory and results that must
 * leave it, overlapped with the extraction of other slots.
 * orbx_host_alloc / orbx_host_free: page-locked host memory (the copies below
 * overlap device work only from such memory).
 * orbx_dev_upload_async: like orbx_dev_upload, but queued on an internal copy
 * stream and returning at once; the copy waits for the extractions queued
 * before the call (which may still read the slots' previous frames), and a
 * later extraction of these slots waits for the copy.  The frame size must be
 * the context's current one (otherwise the call is orbx_dev_upload).
 * orbx_dev_download_async: queue read-backs of slots [first, first+count)
 * after their queued extraction and match: keypoints (count x nfeatures
 * records, slot-major), descriptors (count x nfeatures x 32), keypoint counts
 * (count), match vectors (count x nfeatures) and match counts (count); any
 * pointer may be NULL.  A later extraction of these slots waits for the
 * copies; the host buffers are complete after orbx_dev_sync. */
int  orbx_host_alloc(size_t bytes, void** out);
void orbx_host_free(void* p);
int  orbx_dev_upload_async(orbx_ctx* ctx, int first, int count, const uint8_t* imgs,
                           int w, int h, size_t stride);
int  orbx_dev_download_async(orbx_ctx* ctx, int first, int count, orbx_keypoint* kps,
                             uint8_t* desc, int32_t* n_kps, int32_t* matches12,
                             int32_t* n_matches);
/* Read back one slot's features / its match result (after sync). */
int orbx_dev_read_features(orbx_ctx* ctx, int slot, orbx_keypoint* kps,
                           uint8_t* desc, int cap, int* n_out);
int orbx_dev_read_matches(orbx_ctx* ctx, int slot, int32_t* matches12, int cap,
                          int* n_matches, int* n1);
/* Timing of the dominant kernels over the launches issued since the last
 * reset, measured with hipEvents on the context stream.  name: "pyr0",
 * "resize", "fast", "retain", "blur", "describe", "match", "init" (the three kernels of
 * orbx_init_models / orbx_dev_init_models, one timed region per call),
 * "triangulate" (k_triangulate: one launch per orbx_triangulate_matches or
 * unchained create_new_map_points call, one per neighbour when chained),
 * "sim3" (the three kernels of orbx_sim3_ransac / _batch /
 * orbx_dev_sim3_candidates, one timed region per call; "sim3.prepare",
 * "sim3.solve", "sim3.check": each kernel on its own), "pnp" (the kernels of
 * orbx_pnp_ransac / _batch / orbx_dev_pnp_candidates, one timed region per
 * call; "pnp.prepare", "pnp.solve", "pnp.check", "pnp.refine": the parts on
 * their own, the last with the final selection), "sim3opt" (the one kernel
 * of orbx_optimize_sim3 / _batch / orbx_dev_optimize_sim3).  Returns the
 * number of timed launches; *avg_ms receives the mean duration. */
int orbx_dev_kernel_time(orbx_ctx* ctx, const char* name, double* avg_ms,
                         double* total_ms);
int orbx_dev_kernel_time_enable(orbx_ctx* ctx, int enable);
/* Restrict kernel timing to the launches of one timer name (NULL or "":
 * all), so a timed region carries only the events it reports. */
int orbx_dev_kernel_time_select(orbx_ctx* ctx, const char* name);

/* Debug / parity taps: padded pyramid level (raw or blurred) of a slot.
 * Writes (w_l+32)*(h_l+32) bytes; *pw, *ph receive the padded size.  The
 * extraction keeps only the raw pyramid (the describe kernel blurs each
 * keypoint's patch): a blurred level is computed by this call, from the raw
 * pyramid the slot holds now. */
int orbx_dev_read_level(orbx_ctx* ctx, int slot, int level, int blurred,
                        uint8_t* out, int cap, int* pw, int* ph);

/* ------------------------------------------------------------------------ */
/* B. Matching                                                               */
/* ------------------------------------------------------------------------ */

/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1794-1810), host side. */
int orbx_descriptor_distance(const uint8_t* a, const uint8_t* b);

/* Frame view consumed by the matchers: mvKeysUn, mDescriptors, image bounds
 * (Frame::ComputeImageBounds, src/Frame.cc:320-348) and the scale pyramid
 * (mvScaleFactors, src/Frame.cc:94-102).  The 64x48 cell grid
 * (src/Frame.cc:108-122) is rebuilt on the device from keys_un. */
typedef struct {
    const orbx_keypoint* keys_un;
    const uint8_t* desc;          /* n x 32 */
    int n;
    float min_x, max_x, min_y, max_y;
    int nlevels;
    float scale_factor;
} orbx_frame_view;

/* All-pairs Hamming (B8 primitive): for every row a of dA, the first index of
 * the smallest distance over dB, that distance and the second smallest value
 * of the multiset of distances (reference best/second rule, ORBmatcher.cc:
 * 640-649).  Distances are DescriptorDistance. */
int orbx_hamming_bf(orbx_ctx* ctx, const uint8_t* dA, int nA, const uint8_t* dB,
                    int nB, int32_t* best_idx, int32_t* best, int32_t* second);
/* Brute-force matcher (C3): best/second rule + accept best <= th_low and
 * best < nnratio*second.  m12[a] = matched b or -1. */
int orbx_match_bf(orbx_ctx* ctx, const uint8_t* dA, int nA, const uint8_t* dB,
                  int nB, int th_low, float nnratio, int32_t* m12, int* n_matches);

/* ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:598-713).
 * prev_matched: 2*F1->n floats (vbPrevMatched), updated in place.
 * matches12: F1->n entries (vnMatches12). */
int orbx_search_for_initialization(orbx_ctx* ctx, const orbx_frame_view* F1,
                                   const orbx_frame_view* F2, float* prev_matched,
                                   int32_t* matches12, int window, float nnratio,
                                   int check_ori, int* n_matches);

/* Initializer::Initialize up to the score ratio (src/Initializer.cc:44-113):
 * the matches compacted in i1 order, the RANSAC sets drawn from the caller's
 * rand() values as DUtils::Random::RandomInt maps them (:80-95), Normalize
 * over all keypoints of each frame (:747-793), and for every iteration
 * ComputeH21 / ComputeF21, H21i = T2inv*Hn*T1 with its inverse, F21i =
 * T2t*Fn*T1, CheckHomography / CheckFundamental (:303-466) and the selection
 * of the first strictly greater score (FindHomography :122-170,
 * FindFundamental :173-221), all on the device.  The caller goes on with
 * `if(RH>0.40)` (:113) and orbx_init_reconstruct below.
 * Everything is the reference's float arithmetic operation by operation but
 * the two cv::SVDecomp null vectors, the 3x3 inverses and the denormalising
 * products, which are FP64 rounded once to float; the
 * sign of Hn / Fn is unspecified (no score or inlier depends on it).
 * Arguments are checked before any device work: a null context or query,
 * max_iter outside 1..1024, a draw below 0, sigma <= 0, or a match index >=
 * n2 is ORBX_ERR_ARG; cap < N is ORBX_ERR_CAPACITY; a frame of more than 4096
 * keypoints ORBX_ERR_UNSUPPORTED.  A pair with N < 8 (the reference would
 * index an empty vector; Tracking calls with N >= 100) returns ORBX_OK with
 * n_matches set, best_h = best_f = -1, SH = SF = 0 and RH = 0/0. */
typedef struct {
    /* in */
    const orbx_keypoint* keys1; int n1;   /* Initializer::mvKeys1 = ReferenceFrame.mvKeysUn */
    const orbx_keypoint* keys2; int n2;   /* CurrentFrame.mvKeysUn                          */
    const int32_t* matches12;             /* n1: vMatches12 (index into keys2, or < 0)      */
    float sigma;                          /* 1.0 (src/Tracking.cc:341)                      */
    int max_iter;                         /* 200                                            */
    const int32_t* draws;                 /* max_iter x 8 successive rand() values, 0..RAND_MAX (2^31-1) */
    /* out */
    int n_matches;                        /* N = mvMatches12.size()                         */
    int best_h, best_f;                   /* winning iteration, -1 if no score exceeded 0   */
    float SH, SF, RH;                     /* scores; RH = SH / (SH + SF) in float           */
    float H21[9], F21[9];                 /* row-major; untouched when best_* is -1         */
    uint8_t* inliers_h; uint8_t* inliers_f; int cap;   /* vbMatchesInliersH / F, by match index i */
    /* optional taps (may be NULL), all [max_iter] leading dimension */
    int32_t* sets;                        /* x 8: mvSets                                    */
    float* Hn; float* Fn;                 /* x 9: ComputeH21 / ComputeF21 results           */
    float* H21_all; float* H12_all; float* F21_all;    /* x 9: what the Check* functions read */
    float* score_h; float* score_f;       /* currentScore of every iteration                */
    float* T1; float* T2;                 /* 9 each: Normalize's matrices                   */
} orbx_init_query;

int orbx_init_models(orbx_ctx* ctx, orbx_init_query* q);
int orbx_init_models_batch(orbx_ctx* ctx, int B, orbx_init_query* qs);   /* one upload, one read-back */

/* Device-resident: pair (slot s-1, slot s) for every s in [first, first+count)
 * with s % seq_len != 0, keypoints as the slots hold them (after
 * orbx_dev_undistort if used), matches12 as orbx_dev_match_prev /
 * orbx_dev_extract_match left them in slot s.  draws: count x max_iter x 8
 * (slot s reads block s - first).  The kernels run asynchronously on the
 * context stream, ordered after a pending async match of these slots (the
 * call returns once the draws are uploaded).  Results stay in HBM until read
 * or until the next run.  orbx_dev_read_init_models fills the out fields and
 * taps of `out` (inliers / cap and the tap pointers are read from it; the in
 * fields are ignored); before a run, on a slot outside the run or on a
 * sequence-start slot it is ORBX_ERR_ARG. */
int orbx_dev_init_models(orbx_ctx* ctx, int first, int count, int seq_len,
                         float sigma, int max_iter, const int32_t* draws);
int orbx_dev_read_init_models(orbx_ctx* ctx, int slot, orbx_init_query* out);

/* The end of Initializer::Initialize (src/Initializer.cc:113-119):
 * ReconstructH (:570-730) or ReconstructF (:468-568) with CheckRT (:796-905),
 * Triangulate (:732-745) and DecomposeE (:907-927), all on the device: the
 * motion hypotheses (8 of Faugeras' decomposition of invK*H21*K, or 4 of
 * DecomposeE on K.t()*F21*K), CheckRT of every hypothesis over every inlier
 * match, and the reference's decision.  Everything is the reference's float
 * arithmetic operation by operation but what goes through OpenCV -- the 3x3
 * SVD, the 4x4 null vector of Triangulate, the float matrix products, norm,
 * dot and determinant -- which DESIGN.md section 4 defines (FP64, rounded
 * once).  The signs and, inside a pair of equal singular values, the columns
 * of the SVD are unspecified; they permute the hypothesis list and nothing
 * else, so n_good, parallax, R_all, t_all and best are in the order the
 * device's own decomposition gives.  The reference's own float expressions
 * (:606-614, :649-651, :867-881) follow orbx_set_fp_contract, read at the call.
 * Arguments are checked before any device work: a null context, query or
 * required pointer, a model outside 0..1, sigma <= 0 or a match index >= n2
 * is ORBX_ERR_ARG; cap < n1 is ORBX_ERR_CAPACITY; a frame of more than 4096
 * keypoints ORBX_ERR_UNSUPPORTED.  N == 0 returns ORBX_OK with ok = 0. */
typedef struct {
    /* in */
    const orbx_keypoint* keys1; int n1;     /* mvKeys1 */
    const orbx_keypoint* keys2; int n2;     /* mvKeys2 */
    const int32_t* matches12;               /* n1, as orbx_init_query */
    const uint8_t* inliers;                 /* N = number of matches12 >= 0: vbMatchesInliers by match index */
    int model;                              /* 0: ReconstructH (M21 = H21), 1: ReconstructF (M21 = F21) */
    const float* M21;                       /* 9, row-major */
    const float* cam;                       /* fx, fy, cx, cy (mK) */
    float sigma;                            /* mSigma: th2 = 4.0*sigma*sigma as the reference forms it */
    float min_parallax; int min_triangulated;   /* 1.0, 50 (:114, :116) */
    /* out */
    int ok;                                 /* the function's return value */
    int n_inliers;                          /* N of :471-474 / :573-576 */
    int n_hyp;                              /* 4 (F), 8 (H), 0 when H returns at :595-598 */
    int best;                               /* winning hypothesis, -1 when !ok */
    float R21[9], t21[3];                   /* untouched when !ok */
    int32_t n_good[8]; float parallax[8];   /* CheckRT's results per hypothesis */
    float* p3d; uint8_t* triangulated; int cap;   /* n1 x 3, n1: vP3D / vbTriangulated of the winner; all zero when !ok */
    /* optional taps (may be NULL) */
    float* svd;                             /* 21: U (9), w (3), Vt (9) of the 3x3 decomposition */
    float* R_all; float* t_all;             /* 8 x 9, 8 x 3 */
    float* v4;                              /* n_hyp x N x 4: Triangulate's null vector, written where inliers[i] */
    float* cos_parallax;                    /* n_hyp x N: NaN where the match did not reach :886 */
} orbx_reconstruct_query;

int orbx_init_reconstruct(orbx_ctx* ctx, orbx_reconstruct_query* q);
int orbx_init_reconstruct_batch(orbx_ctx* ctx, int B, orbx_reconstruct_query* qs);   /* one upload, one read-back */

/* Device-resident, after orbx_dev_init_models on the same slot range: per pair
 * the compacted matches, RH, H21 or F21 and the matching inlier array are read
 * where that run left them; the model is H where RH > rh_threshold in float
 * (the reference compares the float RH with the double 0.40, which the float
 * below 0.40f reproduces for every RH) and F otherwise; sigma is the models
 * run's.  A pair whose models run had no winner (best_h or best_f -1, or
 * N < 8) gives ok = 0 and n_hyp = 0.  The kernels run asynchronously on the
 * context stream; results stay in HBM until read or until the next run (of
 * either kind).  orbx_dev_read_init_reconstruct fills the out fields and taps
 * of `out` (p3d / triangulated / cap and the tap pointers are read from it,
 * the in fields are ignored; cap below the pair's n1 is ORBX_ERR_CAPACITY,
 * the v4 and cos_parallax taps hold n_hyp x N entries with N <= n1) and the
 * model that was chosen; before a run, on a slot outside the run or on a
 * sequence-start slot it is ORBX_ERR_ARG. */
int orbx_dev_init_reconstruct(orbx_ctx* ctx, int first, int count, int seq_len, const float* cam,
                              float rh_threshold, float min_parallax, int min_triangulated);
int orbx_dev_read_init_reconstruct(orbx_ctx* ctx, int slot, orbx_reconstruct_query* out, int* model);

/* ORBmatcher::WindowSearch (src/ORBmatcher.cc:409-516).
 * f1_mp: per F1 keypoint, 1 if F1.mvpMapPoints[i1] is set and not bad.
 * matches21 (out, F2->n): i1 whose map point was assigned to F2 keypoint i2,
 * or -1 (vpMapPointMatches2 / vnMatches21).  max_level < 0 means INT_MAX. */
int orbx_window_search(orbx_ctx* ctx, const orbx_frame_view* F1,
                       const orbx_frame_view* F2, const uint8_t* f1_mp,
                       int window, int min_level, int max_level, float nnratio,
                       int check_ori, int32_t* matches21, int* n_matches);

/* ORBmatcher::SearchByProjection(Frame& F1, Frame& F2, int windowSize,
 * vector<MapPoint*>&) (src/ORBmatcher.cc:519-594).
 * f1_mp_xyz: 3 floats per F1 keypoint (world position of its map point);
 * f1_mp_valid: 1 if the point exists, is not bad and is not already in F2
 * (spMapPointsAlreadyFound).  f2_assigned (in): F2.mvpMapPoints non-null.
 * Tcw2: F2 pose, 12 floats row-major [R|t].  cam: fx, fy, cx, cy.
 * matches21 (out): F1 index assigned to each F2 keypoint or -1 (new only). */
int orbx_search_by_projection_pair(orbx_ctx* ctx, const orbx_frame_view* F1,
                                   const orbx_frame_view* F2,
                                   const float* f1_mp_xyz, const uint8_t* f1_mp_valid,
                                   const uint8_t* f2_assigned, const float* Tcw2,
                                   const float* cam, int window, float nnratio,
                                   int32_t* matches21, int* n_matches);

/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame,
 * float th) (src/ORBmatcher.cc:1507-1620), motion-model tracking.
 * last_mp_xyz / last_mp_valid: per LastFrame keypoint (pMP && !mvbOutlier).
 * cur_assigned (in): CurrentFrame.mvpMapPoints non-null.
 * matches_cur (out, Cur->n): LastFrame index assigned to each current
 * keypoint by this call, or -1. */
int orbx_search_by_projection_motion(orbx_ctx* ctx, const orbx_frame_view* Cur,
                                     const orbx_frame_view* Last,
                                     const float* last_mp_xyz,
                                     const uint8_t* last_mp_valid,
                                     const uint8_t* cur_assigned, const float* Tcw,
                                     const float* cam, float th, int check_ori,
                                     int32_t* matches_cur, int* n_matches);

/* ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>&, float th)
 * (src/ORBmatcher.cc:49-125), local-map tracking.  Per map point m (n_mp):
 * in_view (mbTrackInView && !isBad), proj_xy (mTrackProjX/Y), pred_level
 * (mnTrackScaleLevel), view_cos (mTrackViewCos), mp_desc (32 B).
 * f_assigned (in): F.mvpMapPoints non-null.  matches_f (out, F->n): index of
 * the map point assigned to each keypoint by this call, or -1. */
int orbx_search_by_projection_local(orbx_ctx* ctx, const orbx_frame_view* F,
                                    int n_mp, const uint8_t* in_view,
                                    const float* proj_xy, const int32_t* pred_level,
                                    const float* view_cos, const uint8_t* mp_desc,
                                    const uint8_t* f_assigned, float th, float nnratio,
                                    int32_t* matches_f, int* n_matches);

/* Tracking::SearchReferencePointsInFrustum (src/Tracking.cc:701-752) without a
 * host pass over the local map: Frame::isInFrustum(pMP, view_cos_limit)
 * (src/Frame.cc:136-197) for every local map point on the device, then
 * ORBmatcher(nnratio).SearchByProjection(F, mvpLocalMapPoints, th)
 * (src/ORBmatcher.cc:49-125) over the points found in view.  The frame's
 * pose matrices are Frame state (UpdatePoseMatrices, src/Frame.cc:129-134)
 * and are passed as such.  Outputs per point are what isInFrustum writes into
 * the MapPoint (mbTrackInView, mTrackProjX/Y, mnTrackScaleLevel,
 * mTrackViewCos); the caller applies IncreaseVisible() to the points in view
 * and the matches to mvpMapPoints, as the reference's loops do. */
typedef struct {
    const orbx_frame_view* frame;   /* F: mvKeysUn, mDescriptors, bounds, scale pyramid   */
    const float* Rcw;               /* 9, row-major (Frame::mRcw)                          */
    const float* tcw;               /* 3 (mtcw)                                            */
    const float* Ow;                /* 3 (mOw, the camera centre)                          */
    const float* cam;               /* fx, fy, cx, cy                                      */
    int n_mp;                       /* local map points                                    */
    const float* mp_pos;            /* n_mp x 3: GetWorldPos()                             */
    const float* mp_normal;         /* n_mp x 3: GetNormal()                               */
    const float* mp_dist;           /* n_mp x 2: GetMinDistanceInvariance(), GetMaxDistanceInvariance() */
    const uint8_t* mp_skip;         /* n_mp or NULL: 1 = not projected (isBad(), or
                                       mnLastFrameSeen == this frame: already matched)    */
    const uint8_t* mp_desc;         /* n_mp x 32: GetDescriptor()                          */
    const uint8_t* f_assigned;      /* F->n: mvpMapPoints non-null                         */
    float view_cos_limit;           /* 0.5 (src/Tracking.cc:738)                           */
    float th;                       /* 1, or 5 just after relocalisation (:745-748)        */
    float nnratio;                  /* 0.8 (:744)                                          */
    uint8_t* in_view;               /* out, n_mp or NULL: mbTrackInView                    */
    float* proj_xy;                 /* out, n_mp x 2 or NULL: mTrackProjX/Y                */
    int32_t* pred_level;            /* out, n_mp or NULL: mnTrackScaleLevel                */
    float* view_cos;                /* out, n_mp or NULL: mTrackViewCos                    */
    int32_t* matches_f;             /* out, F->n: map point assigned to each keypoint, or -1 */
    int n_in_view;                  /* out: points in view (nToMatch)                      */
    int n_matches;                  /* out: SearchByProjection's return value              */
} orbx_local_map_query;

int orbx_search_local_map(orbx_ctx* ctx, orbx_local_map_query* q);

/* One Tracking frame on the device (Tracking::TrackWithMotionModel then
 * Tracking::TrackLocalMap, src/Tracking.cc:573-600, 604-627): the current
 * frame's keypoints are read where extraction left them (slot `slot`; with
 * `image` set, the image is uploaded and extracted into that slot first),
 * and the chain
 *   SearchByProjection(current, last, 15)            (src/ORBmatcher.cc:1507)
 *   -> < 20 matches: status 1 (the reference then tries TrackPreviousFrame)
 *   -> PoseOptimization, outliers discarded          (src/Optimizer.cc:154)
 *   -> < 10 matches left: status 2
 *   -> SearchReferencePointsInFrustum: isInFrustum of the local map points
 *      not already matched, SearchByProjection(F, local map, th)
 *   -> PoseOptimization on all matches
 * (mode 0) or, mode 1, TrackPreviousFrame's
 *   WindowSearch(last, current, 200, minOctave), < 10: WindowSearch(100)
 *   -> >= 10: PoseOptimization from mLastFrame.mTcw, outliers discarded,
 *      SearchByProjection(last, current, 15); else SearchByProjection(.., 50)
 *   -> < 10 matches: status 3; PoseOptimization, outliers discarded; < 10: 4
 * followed by the same local-map search and PoseOptimization,
 * runs without a host round trip: one upload (last frame, local map, pose
 * prediction, image) and one read-back.  The last frame's map points are
 * named by their index in the map-point arrays.  The local map is an input:
 * the reference rebuilds it (UpdateReference, src/Tracking.cc:754-790) from
 * the keyframes that observe the motion search's matches, between the two
 * searches; a caller passes the one it holds (the previous frame's), which
 * is the reference's whenever those keyframes are unchanged, or runs the two
 * halves with the host-array calls (orbx_search_by_projection_motion,
 * orbx_pose_optimization, orbx_search_local_map) around
 * orbx_covis_update_reference, which rebuilds the local map on the device
 * (its lists are not yet read by this call in HBM).  The camera centre for the frustum
 * test is Frame::UpdatePoseMatrices' mOw = -Rcw^T tcw evaluated in float
 * left to right (the adapter's host glue does the same).  The undistorted
 * keypoints of the slot are its extracted keypoints (k1 = 0) or those
 * orbx_dev_undistort wrote; the frame bounds those of
 * orbx_dev_set_image_bounds (default 0..w, 0..h). */
typedef struct {
    int mode;                       /* 0: TrackWithMotionModel (src/Tracking.cc:572-611);
                                       1: TrackPreviousFrame (:497-569, the reference's
                                       fallback after status 1); both then TrackLocalMap  */
    int min_octave;                 /* mode 1: WindowSearch's minOctave (maxOctave / 2 + 1
                                       when KeyFramesInMap() > 5, else 0, :505-507)        */
    int slot;                       /* current frame's slot                                */
    const uint8_t* image;           /* NULL (slot already extracted) or the mono8 image    */
    int w, h;                       /* image size (also the default bounds)                */
    size_t stride;
    int last_slot;                  /* >= 0: LastFrame is that slot's extraction (the previous
                                       call's slot; `last` unused), else -1              */
    int last_cap;                   /* last_slot >= 0: entries of last_mp / last_outlier (at
                                       least that frame's n_cur, at most nfeatures)       */
    const orbx_frame_view* last;    /* last_slot < 0: LastFrame's mvKeysUn, mDescriptors,
                                       bounds, pyramid                                    */
    const int32_t* last_mp;         /* local-map index of LastFrame.mvpMapPoints[i], or -1 */
    const uint8_t* last_outlier;    /* LastFrame.mvbOutlier                                */
    int n_mp;                       /* map points of the arrays below                      */
    int n_local_mp;                 /* the first n_local_mp of them are mvpLocalMapPoints (the
                                       frustum search's); the rest only LastFrame's. <= 0: all */
    const float* mp_pos;            /* n_mp x 3                                            */
    const float* mp_normal;         /* n_mp x 3                                            */
    const float* mp_dist;           /* n_mp x 2: min, max distance invariance              */
    const uint8_t* mp_desc;         /* n_mp x 32                                           */
    const uint8_t* mp_skip;         /* n_mp or NULL: isBad()                               */
    const float* Tcw_pred;          /* 12: mode 0 rows 0..2 of mVelocity * mLastFrame.mTcw,
                                       mode 1 of mLastFrame.mTcw                          */
    const float* cam;               /* fx, fy, cx, cy                                      */
    const float* inv_level_sigma2;  /* nlevels (mvInvLevelSigma2)                          */
    int nlevels;
    float th_local;                 /* 1, or 5 just after relocalisation                   */
    /* outputs */
    float Tcw[12];                  /* final pose (rows 0..2): after the last PoseOptimization
                                       that ran (the prediction for status 1)              */
    int32_t* cur_mp;                /* cap: local-map index per current keypoint, or -1     */
    uint8_t* cur_outlier;           /* cap: mvbOutlier after the last PoseOptimization      */
    int cap;                        /* capacity of cur_mp / cur_outlier                    */
    int n_cur;                      /* current frame's keypoints                           */
    int status;                     /* 0 tracked (TrackLocalMap ran); mode 0: 1 / 2 above;
                                       mode 1: 3 < 10 matches after the window and pair
                                       searches, 4 < 10 left after their PoseOptimization */
    int n_motion;                   /* mode 0: SearchByProjection(current, last) matches;
                                       mode 1: the WindowSearch's (200, else 100)         */
    int n_pair;                     /* mode 1: SearchByProjection(last, current, 15 / 50)  */
    int n_after_pose;               /* matches left after the PoseOptimization before the
                                       local-map search                                   */
    int n_in_view;                  /* local map points in view (nToMatch)                  */
    int n_local;                    /* SearchByProjection(F, local map) matches            */
    int n_inliers;                  /* the last PoseOptimization's return value            */
} orbx_track_query;
int orbx_track_frame(orbx_ctx* ctx, orbx_track_query* q);
/* B independent frames (each with its own local map) in one upload, two
 * launches (all frustum tests, then one search wavefront per frame) and one
 * readback. */
int orbx_search_local_map_batch(orbx_ctx* ctx, int B, orbx_local_map_query* qs);

/* Vocabulary-node searches.  A keyframe or frame as
 * the BoW matchers read it: keypoints (angle; pt and octave for the
 * epipolar test), descriptors, the map-point state of every keypoint and
 * its DBoW2::FeatureVector (node id -> feature indices, std::map order) as
 * CSR arrays.  mp: 0 = no map point, 1 = map point, 2 = map point isBad().
 * Every feature index appears in at most one node (DBoW2 transform). */
typedef struct {
    const orbx_keypoint* keys;      /* [n] mvKeysUn (Frame side of
                                       SearchByBoW(KF, F): mvKeys)          */
    const uint8_t* desc;            /* [n][32] mDescriptors                  */
    int n;
    const uint8_t* mp;              /* [n] map-point state                   */
    int n_nodes;                    /* FeatureVector entries                 */
    const uint32_t* node_id;        /* [n_nodes] ascending                   */
    const int32_t* node_ptr;        /* [n_nodes + 1] offsets into feat_idx   */
    const int32_t* feat_idx;        /* feature indices of each node, as stored */
} orbx_bow_view;

/* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>&)
 * (src/ORBmatcher.cc:155-283).  matches_f (out, F->n): the KF keypoint whose
 * map point was assigned to each F keypoint (vpMapPointMatches), or -1. */
int orbx_search_by_bow_frame(orbx_ctx* ctx, const orbx_bow_view* KF, const orbx_bow_view* F,
                             float nnratio, int check_ori, int32_t* matches_f, int* n_matches);
/* ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>&)
 * (src/ORBmatcher.cc:715-850).  matches12 (out, KF1->n): the KF2 keypoint
 * whose map point matched each KF1 keypoint (vpMatches12), or -1. */
int orbx_search_by_bow_kf(orbx_ctx* ctx, const orbx_bow_view* KF1, const orbx_bow_view* KF2,
                          float nnratio, int check_ori, int32_t* matches12, int* n_matches);
/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, ...) (src/ORBmatcher.cc:
 * 852-1014).  F12: 3x3 row-major fundamental matrix (float, as cv::Mat);
 * sigma2_2: KF2's mvLevelSigma2 (nlevels entries).  matches12 (out, KF1->n):
 * vMatches12 (KF2 index or -1); vMatchedPairs are its non-negative entries
 * in KF1 order. */
int orbx_search_for_triangulation(orbx_ctx* ctx, const orbx_bow_view* KF1, const orbx_bow_view* KF2,
                                  const float* F12, const float* sigma2_2, int nlevels, int check_ori,
                                  int32_t* matches12, int* n_matches);
/* Batched forms for LocalMapping's per-neighbour loops: one keyframe KF1
 * against n keyframes KF2s[k] in one upload, one launch (a workgroup per
 * pair) and one readback; results as n separate calls would give.
 * SearchForTriangulation: CreateNewMapPoints (src/LocalMapping.cc:220-260,
 * F12s n x 9, sigma2_2s n x nlevels).  SearchByBoW(KF1, KF2): the loop
 * candidates of LoopClosing::ComputeSim3 (src/LoopClosing.cc:240).
 * matches12[k] (out, KF1->n) and n_matches[k] per pair. */
int orbx_search_for_triangulation_batch(orbx_ctx* ctx, const orbx_bow_view* KF1, int n,
                                        const orbx_bow_view* KF2s, const float* F12s,
                                        const float* sigma2_2s, int nlevels, int check_ori,
                                        int32_t* const* matches12, int* n_matches);
int orbx_search_by_bow_kf_batch(orbx_ctx* ctx, const orbx_bow_view* KF1, int n, const orbx_bow_view* KF2s,
                                float nnratio, int check_ori, int32_t* const* matches12, int* n_matches);

/* Keyframe projection searches.  Map points as they
 * read them, one entry per point (SoA). */
typedef struct {
    int n;
    const float* pos;        /* [n][3] GetWorldPos()                        */
    const float* normal;     /* [n][3] GetNormal() (Fuse; may be NULL else)  */
    const float* min_dist;   /* [n] GetMinDistanceInvariance()               */
    const float* max_dist;   /* [n] GetMaxDistanceInvariance()               */
    const uint8_t* desc;     /* [n][32] GetDescriptor()                      */
} orbx_mappoint_view;

/* ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>&, th) (src/ORBmatcher.cc:
 * 1016-1134; sim3 = 0, T = the keyframe's Tcw) and Fuse(KeyFrame*, Scw,
 * vector<MapPoint*>&, th) (:1136-1265; sim3 = 1, T = Scw), 4x4 row-major
 * float.  Computes the state-free part for every map point -- projection,
 * image / distance / viewing-angle gates, predicted level, and the best
 * keyframe keypoint within th * scale[level] at levels [pred - 1, pred]:
 * best_idx (-1 when gated out or no candidate) and best_dist.  The caller
 * replays the graph updates in map-point order (isBad / IsInKeyFrame /
 * already-found checks, bestDist <= TH_LOW, Replace or AddObservation),
 * which depend on the earlier points' updates. */
int orbx_fuse_candidates(orbx_ctx* ctx, const orbx_frame_view* KF, const float* cam,
                         const orbx_mappoint_view* mps, const float* T, int sim3, float th,
                         int32_t* best_idx, int32_t* best_dist);
/* Fuse candidates for n keyframes in one upload / launch / readback:
 * SearchInNeighbors' loop over the target keyframes (src/LocalMapping.cc:
 * 403-416), KFs[k] with camera cams[4k..], pose Ts[16k..] and map points
 * *mps[k] (views that are the same object are uploaded once: the loop fuses
 * the current keyframe's points into every neighbour).  The candidates are
 * state-free, so computing all of them before the caller replays the graph
 * updates neighbour by neighbour gives the sequential loop's result (a point
 * replaced or already in the keyframe is skipped at replay, as there). */
int orbx_fuse_candidates_batch(orbx_ctx* ctx, int n_kf, const orbx_frame_view* KFs, const float* cams,
                               const orbx_mappoint_view* const* mps, const float* Ts, int sim3, float th,
                               int32_t* const* best_idx, int32_t* const* best_dist);
/* orbx_fuse_candidates_batch against keyframes that stay in their extraction
 * slots: keyframe k is the frame in slots[k] (keypoints as the slot holds
 * them -- mvKeysUn after orbx_dev_undistort -- descriptors, the extractor's
 * scale pyramid), with image bounds bounds[4k..4k+3] (min_x, max_x, min_y,
 * max_y; Frame::ComputeImageBounds) or, bounds NULL, 0..w x 0..h.  Only the
 * map points, cameras and poses are uploaded; results as the batch form. */
int orbx_dev_fuse_candidates(orbx_ctx* ctx, int n_kf, const int* slots, const float* bounds, const float* cams,
                             const orbx_mappoint_view* const* mps, const float* Ts, int sim3, float th,
                             int32_t* const* best_idx, int32_t* const* best_dist);
/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
 * (src/ORBmatcher.cc:1267-1505).  mp1 / valid1: the map point of each KF1
 * keypoint (valid = pMP && !isBad()); mp2 / valid2 likewise for KF2.  T1w,
 * T2w: keyframe poses (4x4 row-major); R12 3x3 row-major, t12 3.  prior12
 * (in, KF1->n): -2 where vpMatches12[i] is NULL, else the KF2 index of that
 * map point (GetIndexInKeyFrame(pKF2), -1 if not observed).  new12 (out):
 * the KF2 keypoint whose map point this call assigns (vpMatches12[i1] =
 * vpMapPoints2[new12[i1]]), or -1.  cam: pKF1's fx, fy, cx, cy. */
int orbx_search_by_sim3(orbx_ctx* ctx, const orbx_frame_view* KF1, const orbx_frame_view* KF2,
                        const float* cam, const orbx_mappoint_view* mp1, const uint8_t* valid1,
                        const orbx_mappoint_view* mp2, const uint8_t* valid2, const float* T1w,
                        const float* T2w, float s12, const float* R12, const float* t12, float th,
                        const int32_t* prior12, int32_t* new12, int* n_found);
/* The same with both keyframes resident in their extraction slots (keypoints
 * as the slots hold them; bounds1 / bounds2: min_x, max_x, min_y, max_y, or
 * NULL for 0..w x 0..h; mp1 / valid1 / prior12 one entry per slot1 keypoint,
 * mp2 / valid2 per slot2 keypoint).  new12: cap >= slot1's keypoint count. */
int orbx_dev_search_by_sim3(orbx_ctx* ctx, int slot1, const float* bounds1, int slot2, const float* bounds2,
                            const float* cam, const orbx_mappoint_view* mp1, const uint8_t* valid1,
                            const orbx_mappoint_view* mp2, const uint8_t* valid2, const float* T1w,
                            const float* T2w, float s12, const float* R12, const float* t12, float th,
                            const int32_t* prior12, int32_t* new12, int cap, int* n_found);
/* ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const
 * vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, int th)
 * (src/ORBmatcher.cc:286-407), loop closing.  mps: vpPoints; mp_skip:
 * pMP->isBad() or already in vpMatched (spAlreadyFound).  matched (in/out,
 * KF->n): vpMatched as an index into mps (any value >= 0 for an entry set by
 * the caller), -1 where NULL; the call writes the entries it assigns. */
int orbx_search_by_projection_kf_sim3(orbx_ctx* ctx, const orbx_frame_view* KF, const float* cam,
                                      const orbx_mappoint_view* mps, const uint8_t* mp_skip,
                                      const float* Scw, int th, int32_t* matched, int* n_matches);
/* The same against a keyframe resident in its extraction slot (keypoints as
 * the slot holds them, mvKeysUn after orbx_dev_undistort; bounds: min_x,
 * max_x, min_y, max_y, or NULL for 0..w x 0..h).  matched (in / out): cap >=
 * the slot's keypoint count entries, as above. */
int orbx_dev_search_by_projection_kf_sim3(orbx_ctx* ctx, int slot, const float* bounds, const float* cam,
                                          const orbx_mappoint_view* mps, const uint8_t* mp_skip, const float* Scw,
                                          int th, int32_t* matched, int cap, int* n_matches);
/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const
 * set<MapPoint*>& sAlreadyFound, float th, int ORBdist) (src/ORBmatcher.cc:
 * 1622-1746), relocalisation.  KF: pKF's keypoints (mvKeysUn); kf_mps: the
 * map point of each KF keypoint (pos, min_dist, desc); kf_valid: pMP &&
 * !isBad() && !sAlreadyFound.count(pMP).  F: CurrentFrame; f_assigned:
 * CurrentFrame.mvpMapPoints[i] != NULL; Tcw: CurrentFrame.mTcw (4x4
 * row-major); cam: CurrentFrame's fx, fy, cx, cy.  matches_f (out, F->n):
 * the KF keypoint whose map point this call assigns, or -1. */
int orbx_search_by_projection_frame_kf(orbx_ctx* ctx, const orbx_frame_view* F, const orbx_frame_view* KF,
                                       const float* cam, const orbx_mappoint_view* kf_mps,
                                       const uint8_t* kf_valid, const uint8_t* f_assigned,
                                       const float* Tcw, float th, int orb_dist, int check_ori,
                                       int32_t* matches_f, int* n_matches);
/* The same with the current frame in f_slot (bounds: min_x, max_x, min_y,
 * max_y, or NULL for 0..w x 0..h) and the candidate keyframe in kf_slot
 * (its keypoints from the slot; kf_mps / kf_valid: one entry per keyframe
 * keypoint), both as extraction / orbx_dev_undistort left them.
 * matches_f: cap >= the frame's keypoint count entries. */
int orbx_dev_search_by_projection_frame_kf(orbx_ctx* ctx, int f_slot, const float* f_bounds, int kf_slot,
                                           const float* cam, const orbx_mappoint_view* kf_mps,
                                           const uint8_t* kf_valid, const uint8_t* f_assigned, const float* Tcw,
                                           float th, int orb_dist, int check_ori, int32_t* matches_f, int cap,
                                           int* n_matches);
/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:185-250) for
 * n_mp map points at once: point m's observed descriptors (non-bad
 * keyframes, observation order) are rows obs_ptr[m] .. obs_ptr[m+1]-1 of
 * desc.  best (out): the row (relative to obs_ptr[m]) with the least median
 * distance to the others, -1 for a point without descriptors. */
int orbx_distinctive_descriptors(orbx_ctx* ctx, int n_mp, const int32_t* obs_ptr,
                                 const uint8_t* desc, int32_t* best);

/* Frame construction.  Frame::UndistortKeyPoints
 * (src/Frame.cc:288-318): cv::undistortPoints with P = K, K = (fx, fy, cx,
 * cy), dist = (k1, k2, p1, p2, k3) (mDistCoef; k3 = 0 for 4 coefficients).
 * A zero k1 copies the keypoints (:290-294), as the reference does. */
int orbx_undistort_keypoints(orbx_ctx* ctx, int n, const orbx_keypoint* keys, const float* K,
                             const float* dist, orbx_keypoint* keys_un);
/* Frame::ComputeImageBounds (src/Frame.cc:320-348): bounds = mnMinX,
 * mnMaxX, mnMinY, mnMaxY for a w x h image (host only, four points). */
int orbx_compute_image_bounds(int w, int h, const float* K, const float* dist, float* bounds);
/* Device-resident form: undistort the keypoints of extracted slots
 * [first, first+count) in place (after orbx_dev_extract, before matching). */
int orbx_dev_undistort(orbx_ctx* ctx, int first, int count, const float* K, const float* dist);

/* DBoW2 vocabulary: the tree as
 * TemplatedVocabulary::loadFromTextFile builds it (Thirdparty/DBoW2/DBoW2/
 * TemplatedVocabulary.h:1338-1420) -- node 0 the root, node i (1..n-1) a
 * child of parent[i] (children in increasing id order), word ids given to
 * the nodes flagged is_leaf in id order, a 32-byte descriptor and a weight
 * (idf) per node.  Kept in HBM for the vocabulary's lifetime.  A refused
 * call (ORBX_ERR_ARG: a null pointer, k, L < 1, n_nodes < 2, a parent[i]
 * outside [0, i)) leaves *out NULL. */
typedef struct orbx_vocab orbx_vocab;
int orbx_vocab_create(orbx_ctx* ctx, int k, int L, int n_nodes, const int32_t* parent,
                      const uint8_t* is_leaf, const uint8_t* desc, const double* weight,
                      orbx_vocab** out);
void orbx_vocab_destroy(orbx_vocab* voc);
int orbx_vocab_n_words(const orbx_vocab* voc);
/* TemplatedVocabulary::transform(features, BowVector&, FeatureVector&,
 * levelsup) (:1127-1259) as Frame::ComputeBoW calls it (src/Frame.cc:
 * 279-286, levelsup 4), TF-IDF weighting with L1 scoring (ORBvoc.txt's).
 * The tree descent of the n descriptors runs on the device; per feature:
 * word_id, weight and the level-(L - levelsup) node (node_id, -1 if the
 * descent ended above that level).  BowVector: n_words (word, value) pairs,
 * words ascending, values L1-normalised.  FeatureVector: n_fv_nodes node
 * ids ascending with CSR offsets fv_ptr (n_fv_nodes + 1) into fv_feat.
 * Stopped words (weight 0) are left out of both.  Capacities: n entries
 * (fv_ptr: n + 1). */
int orbx_vocab_transform(orbx_ctx* ctx, const orbx_vocab* voc, int n, const uint8_t* desc,
                         int levelsup, int32_t* word_id, double* weight, int32_t* node_id,
                         uint32_t* bow_words, double* bow_values, int* n_words,
                         uint32_t* fv_nodes, int32_t* fv_ptr, int32_t* fv_feat, int* n_fv_nodes);

/* Device-resident form for extracted slots: Frame::ComputeBoW (src/Frame.cc:
 * 279-286) of slots [first, first+count) -- the descent of every extracted
 * descriptor and the slot's BowVector / FeatureVector built on the device,
 * kept in HBM until the slot is extracted again (async, context stream).
 * Frames of up to 4096 features (ORBX_ERR_UNSUPPORTED above). */
int orbx_dev_compute_bow(orbx_ctx* ctx, const orbx_vocab* voc, int first, int count, int levelsup);
/* Read one slot's BoW (after orbx_dev_compute_bow; syncs), the arrays of
 * orbx_vocab_transform with the same meaning.  Any output may be NULL;
 * cap >= the slot's feature count (ORBX_ERR_CAPACITY otherwise). */
int orbx_dev_read_bow(orbx_ctx* ctx, int slot, int cap, int32_t* word_id, double* weight, int32_t* node_id,
                      uint32_t* bow_words, double* bow_values, int* n_words, uint32_t* fv_nodes,
                      int32_t* fv_ptr, int32_t* fv_feat, int* n_fv_nodes);
/* Tracking::Relocalisation's matching loop (src/Tracking.cc:904-925):
 * ORBmatcher::SearchByBoW(pKF, F) (src/ORBmatcher.cc:155-283) of n
 * candidate keyframes against the frame in `slot`, its keypoints,
 * descriptors and FeatureVector read where orbx_dev_extract /
 * orbx_dev_compute_bow left them.  matches_f[k] (cap >= nfeatures entries):
 * per frame keypoint the KF keypoint index or -1, as orbx_search_by_bow_frame. */
int orbx_dev_search_by_bow(orbx_ctx* ctx, int slot, int n, const orbx_bow_view* KFs, float nnratio,
                           int check_ori, int32_t* const* matches_f, int cap, int* n_matches);
/* The keyframe-pair searches between device-resident frames, the keyframe
 * in slot1 against those in slots2[0, n) (keypoints as the slots hold them,
 * mvKeysUn after orbx_dev_undistort; FeatureVectors from
 * orbx_dev_compute_bow on every slot named): SearchByBoW(KF1, KF2)
 * (src/ORBmatcher.cc:715-850) as LoopClosing::ComputeSim3's candidate loop
 * (src/LoopClosing.cc:240) runs it, and SearchForTriangulation (:852-1014)
 * as LocalMapping::CreateNewMapPoints' neighbour loop (src/LocalMapping.cc:
 * 220-260) does (F12s n x 9, sigma2_2s n x nlevels, nlevels the
 * extractor's).  Only the map-point states travel: mp1 and mp2s[k] hold one
 * state per keypoint of the slot (0 none, 1 map point, 2 isBad()).
 * matches12[k] (cap >= nfeatures entries): per slot1 keypoint the slots2[k]
 * keypoint or -1, as the host-array forms. */
int orbx_dev_search_by_bow_kf(orbx_ctx* ctx, int slot1, const uint8_t* mp1, int n, const int* slots2,
                              const uint8_t* const* mp2s, float nnratio, int check_ori,
                              int32_t* const* matches12, int cap, int* n_matches);
int orbx_dev_search_for_triangulation(orbx_ctx* ctx, int slot1, const uint8_t* mp1, int n, const int* slots2,
                                      const uint8_t* const* mp2s, const float* F12s, const float* sigma2_2s,
                                      int nlevels, int check_ori, int32_t* const* matches12, int cap,
                                      int* n_matches);

/* New map points: LocalMapping::CreateNewMapPoints' neighbour loop
 * (src/LocalMapping.cc:245-385) behind its SearchForTriangulation call.  The
 * baseline test (:249-258), ComputeF12 and `new MapPoint ...
 * UpdateNormalAndDepth` (:370-383) stay with the caller. */
typedef struct {                 /* a keyframe as CreateNewMapPoints reads it */
    const float* Rcw;            /* 9  GetRotation(), row-major   */
    const float* tcw;            /* 3  GetTranslation()           */
    const float* Ow;             /* 3  GetCameraCenter()          */
    const float* cam;            /* fx, fy, cx, cy                */
    const float* scale_factors;  /* nlevels: mvScaleFactors       */
    const float* level_sigma2;   /* nlevels: mvLevelSigma2        */
    int nlevels;                 /* >= 2 (ratioFactor reads [1])  */
} orbx_kf_geom;

/* The per-match half of the loop (:283-368) for the matches of KF1 against
 * n neighbours: matches12[k] holds per KF1 keypoint a keys2[k] index or < 0.
 * One upload, one launch over all (k, i1), one read-back.  Per neighbour:
 * status[k] (n1 bytes, all written):
 *   0 no match for this keypoint      5 z2 <= 0 (:327)
 *   1 point created, xyz holds x3D    6 reprojection error in KF1 (:339)
 *   2 parallax gate (:299)            7 reprojection error in KF2 (:351)
 *   3 x3D(3) == 0 (:314)              8 dist1 == 0 || dist2 == 0 (:361)
 *   4 z1 <= 0 (:323)                  9 scale consistency (:366)
 * xyz[k] (n1 x 3, written where status is 1), n_created[k], and the optional
 * tap v4[k] (n1 x 4, v4 or v4[k] may be NULL): the null vector of A, written
 * where the solve ran (status neither 0 nor 2).
 * The gates are the reference's float arithmetic operation by operation;
 * OpenCV's double accumulations and the cv::SVD null vector -- FP64 from the
 * float entries of A, rounded once, sign unspecified (the division by x3D(3)
 * is sign-invariant) -- are the defined parts of DESIGN.md section 4.
 * ORBX_ERR_ARG (before any device work): a null context or required pointer,
 * nlevels outside 2..16, an octave >= its keyframe's nlevels, a match index
 * >= n2s[k].  n == 0 or n1 == 0 returns ORBX_OK and touches nothing. */
int orbx_triangulate_matches(orbx_ctx* ctx, const orbx_keypoint* keys1, int n1, const orbx_kf_geom* g1, int n,
                             const orbx_keypoint* const* keys2, const int* n2s, const orbx_kf_geom* g2s,
                             const int32_t* const* matches12, float* const* xyz, uint8_t* const* status,
                             int* n_created, float* const* v4);
/* The loop: SearchForTriangulation of KF1 against KF2s[0, n) (views, F12s
 * and check_ori as orbx_search_for_triangulation_batch; KF2's mvLevelSigma2
 * from g2s) and the triangulation of its matches, in one call.  matches12[k]
 * (KF1->n entries) and n_matches[k] as the search returns them, the rest as
 * orbx_triangulate_matches.
 * chain = 0: every neighbour is searched with the caller's map-point states:
 *   the batch search followed by orbx_triangulate_matches, bit for bit.
 * chain = 1: the reference's loop.  A point created for a KF1 keypoint
 *   against neighbour k gives it a map point (:375), so the searches of the
 *   neighbours after k skip it (src/ORBmatcher.cc:894-896) and its candidate
 *   there stays free for other keypoints.  The n searches and triangulations
 *   are queued on the context stream, neighbour after neighbour, without a
 *   host synchronisation in between.  A created point changes KF2's states
 *   as well (:376): a KF2 listed twice (the same keys or mp array) is
 *   ORBX_ERR_ARG. */
int orbx_create_new_map_points(orbx_ctx* ctx, const orbx_bow_view* KF1, const orbx_kf_geom* g1, int n,
                               const orbx_bow_view* KF2s, const orbx_kf_geom* g2s, const float* F12s,
                               int check_ori, int chain, int32_t* const* matches12, int* n_matches,
                               float* const* xyz, uint8_t* const* status, int* n_created, float* const* v4);
/* The same between device-resident frames, with the inputs of
 * orbx_dev_search_for_triangulation: only the map-point states, F12s and the
 * geometries travel.  Every geometry must have the extractor's nlevels
 * (ORBX_ERR_ARG otherwise).  Every output array holds cap >= nfeatures
 * entries (ORBX_ERR_CAPACITY below): matches12[k] cap, status[k] cap (0 past
 * the slot's keypoints), xyz[k] cap x 3, v4[k] cap x 4.  A match whose index
 * or octave is out of range is dropped as status 0.  A slot listed twice in
 * slots2 under chain = 1 is ORBX_ERR_ARG. */
int orbx_dev_create_new_map_points(orbx_ctx* ctx, int slot1, const uint8_t* mp1, const orbx_kf_geom* g1, int n,
                                   const int* slots2, const uint8_t* const* mp2s, const orbx_kf_geom* g2s,
                                   const float* F12s, int check_ori, int chain, int32_t* const* matches12,
                                   int* n_matches, float* const* xyz, uint8_t* const* status, int* n_created,
                                   float* const* v4, int cap);

/* Sim3Solver (src/Sim3Solver.cc): Horn's closed-form similarity inside a
 * RANSAC over the matches of two keyframes, step 2 of
 * LoopClosing::ComputeSim3 (src/LoopClosing.cc:231-344) between
 * orbx_search_by_bow_kf_batch and orbx_search_by_sim3.  One call is one
 * Sim3Solver::iterate(n_iter, ...) (:140-207) of a solver built by the
 * constructor (:37-112) and SetRansacParameters (:114-138): the
 * correspondences compacted in i1 order, the camera coordinates, their
 * projections and the integer error limits, then every iteration of the
 * call at once -- its minimal set from the caller's rand() values (with the
 * reference's removal at the drawn value's position, :175), computeT
 * (:226-332) and CheckInliers (:335-359) -- and the replay of the loop's
 * sequential bookkeeping over the inlier counts.
 * A correspondence is kept for i1 when matches12[i1] >= 0, k1 = idx1 ?
 * idx1[i1] : i1 lies in [0, n1) (GetIndexInKeyFrame(pKF1) >= 0), valid1[k1]
 * and valid2[matches12[i1]] are set (a map point that is not isBad()); it
 * reads pos1[k1], keys1[k1].octave, pos2[i2], keys2[i2].octave.
 * The float arithmetic the reference writes itself is followed operation by
 * operation (fx*x+cx follows orbx_set_fp_contract); the places that go
 * through OpenCV, and the quaternion -- the unit eigenvector of N for its
 * largest eigenvalue, FP64 from the float entries, rounded once, q0 >= 0 --
 * are defined in DESIGN.md section 4.
 * The iterations of a call are [iter_done, iter_done + n_iter) of the
 * solver, cut at ransac_max_its.  The call returns like iterate: at the first
 * iteration whose count reaches the running best (which starts at
 * best_inliers) and exceeds min_inliers -- found = 1, found_iter its index in
 * this call, iters_run = found_iter + 1; the caller continues a solver with
 * iter_done + iters_run, best_inliers_out and the draws that follow.
 * Arguments are checked before any device work.  ORBX_ERR_ARG: a null
 * context, query or required pointer, n_iter outside 1..1024, a draw < 0,
 * min_inliers < 3, max_iterations < 1, iter_done or best_inliers < 0, a
 * probability outside (0,1), nlevels outside 1..16, an octave outside
 * [0, nlevels), a level sigma2 that is negative, not finite or whose limit
 * 9.210 * sigma2 does not fit an int, a match index >= n2, an idx1 entry >= n1;
 * ORBX_ERR_UNSUPPORTED: more than 4096 keypoints; ORBX_ERR_CAPACITY: cap <
 * n1.  N < min_inliers returns ORBX_OK with no_more = 1, found = 0 and no
 * iteration run (:146-150). */
typedef struct {
    /* in */
    const orbx_keypoint* keys1; int n1;   /* pKF1's mvKeysUn (the octave is read)             */
    const orbx_keypoint* keys2; int n2;   /* pKF2's                                           */
    const int32_t* matches12;             /* n1: KF2 keypoint of vpMatched12[i1], or < 0      */
    const int32_t* idx1;                  /* n1: GetIndexInKeyFrame(pKF1) of pKF1's map point
                                             at i1 (< 0: none); NULL: i1                      */
    const float* pos1; const uint8_t* valid1;   /* n1 x 3 GetWorldPos(), n1: 1 = a good map point */
    const float* pos2; const uint8_t* valid2;   /* n2 x 3, n2                                     */
    const float* T1w; const float* T2w;   /* 16 each: the keyframes' Tcw, row-major           */
    const float* cam1; const float* cam2; /* fx, fy, cx, cy                                   */
    const float* sigma2_1; const float* sigma2_2; int nlevels;   /* mvLevelSigma2 of each     */
    double probability; int min_inliers; int max_iterations;     /* 0.99, 20, 300 (LoopClosing.cc:276) */
    /* iterate state (in) */
    int iter_done;                        /* mnIterations on entry                            */
    int best_inliers;                     /* mnBestInliers on entry                           */
    int n_iter;                           /* iterate's nIterations (find(): the cap)          */
    const int32_t* draws;                 /* n_iter x 3 successive rand() values              */
    /* out */
    int N;                                /* correspondences                                  */
    int ransac_max_its;                   /* mRansacMaxIts (0 when N < min_inliers, where the
                                             reference converts a NaN)                        */
    int iters_run;                        /* iterations executed by this call                 */
    int no_more;                          /* bNoMore                                          */
    int found, found_iter;                /* a non-empty return; its iteration or -1          */
    int n_inliers;                        /* nInliers (0 when !found)                         */
    float T12[16];                        /* the returned mBestT12 (untouched when !found)    */
    uint8_t* inliers; int cap;            /* vbInliers by i1 (n1 written, all 0 when !found)  */
    int best_inliers_out;                 /* mnBestInliers at return                          */
    int best_iter;                        /* the iteration of this call that holds the mBest*
                                             state at return, -1: none reached best_inliers   */
    float R12[9], t12[3], s12;            /* mBestRotation / Translation / Scale (untouched
                                             when best_iter is -1)                            */
    /* optional taps (may be NULL), leading dimension n_iter */
    int32_t* sets;                        /* x 3: indices into the correspondences            */
    float* q;                             /* x 4: the quaternion (w, x, y, z)                 */
    float* R; float* scale;               /* x 9: mR12i; ms12i                                */
    float* T12_all; float* T21_all;       /* x 16                                             */
    int32_t* count;                       /* mnInliersi                                       */
    /* optional taps per correspondence (cap >= n1 entries each, N written) */
    float* x3dc1; float* x3dc2;           /* x 3: mvX3Dc1 / 2                                 */
    float* p1im1; float* p2im2;           /* x 2: mvP1im1 / mvP2im2                           */
    int32_t* max_err1; int32_t* max_err2; /* mvnMaxError1 / 2                                 */
    int32_t* indices1;                    /* mvnIndices1                                      */
} orbx_sim3_query;

int orbx_sim3_ransac(orbx_ctx* ctx, orbx_sim3_query* q);   /* one upload, one read-back */
/* ComputeSim3's candidates in one upload, one launch set and one read-back;
 * results as B single calls. */
int orbx_sim3_ransac_batch(orbx_ctx* ctx, int B, orbx_sim3_query* qs);

/* A device-resident keyframe as the solver reads it: what does not live in
 * the slot. */
typedef struct {
    const uint8_t* mp;       /* per keypoint: 0 none, 1 map point, 2 isBad() (as orbx_dev_search_by_bow_kf) */
    const float* pos;        /* per keypoint x 3: GetWorldPos() (read where mp is 1)                          */
    const float* Tcw;        /* 16                                                                            */
    const float* cam;        /* fx, fy, cx, cy                                                                */
    const float* sigma2;     /* nlevels: mvLevelSigma2                                                        */
    int nlevels;             /* the extractor's                                                               */
} orbx_sim3_kf;

/* Steps 1 and 2 of ComputeSim3 between device-resident frames: SearchByBoW
 * (KF1 in slot1, KF2 in slots2[k]) as orbx_dev_search_by_bow_kf queues it,
 * and on the match vectors where the search left them a fresh Sim3Solver per
 * candidate (idx1 = i1; the iterate state is read from out[k]: iter_done,
 * best_inliers) running n_iter iterations from draws (n x n_iter x 3).  A
 * candidate with n_matches[k] < min_matches (20, LoopClosing.cc:268) is
 * discarded[k] = 1 and runs no RANSAC (its out fields read N = 0, found = 0,
 * no_more = 0).  One synchronisation and one read-back: matches12[k] (cap >=
 * nfeatures entries), n_matches[k], discarded[k] and out[k]'s out fields and
 * taps (out[k].inliers / cap >= nfeatures and the tap pointers are read from
 * it; its other in fields are ignored).  Results as
 * orbx_dev_search_by_bow_kf followed by orbx_sim3_ransac_batch on the
 * read-back matches.  A match whose index or octave is out of range is
 * dropped.  The mp / pos arrays hold one entry per keypoint of the slot. */
int orbx_dev_sim3_candidates(orbx_ctx* ctx, int slot1, const orbx_sim3_kf* kf1, int n, const int* slots2,
                             const orbx_sim3_kf* kf2s, float nnratio, int check_ori, int min_matches,
                             double probability, int min_inliers, int max_iterations, int n_iter,
                             const int32_t* draws, int32_t* const* matches12, int cap, int* n_matches,
                             int* discarded, orbx_sim3_query* out);

/* Optimizer::OptimizeSim3 (src/Optimizer.cc:791-987), step 4 of
 * LoopClosing::ComputeSim3 (src/LoopClosing.cc:328, th2 = 10) between
 * orbx_search_by_sim3 and the final projection search: g2o's Levenberg over
 * one free VertexSim3Expmap (7 DoF, _fix_scale false) against fixed points
 * through an EdgeSim3ProjectXYZ (e12) and an EdgeInverseSim3ProjectXYZ (e21)
 * per correspondence, Huber with delta = sqrtf(th2), BlockSolverX +
 * LinearSolverDense (Eigen LDLT, 7 x 7), numeric central-difference Jacobians
 * with delta 1e-9 (the reference's linearizeOplus is commented out), every sum
 * in g2o's edge order e12_0, e21_0, e12_1, ...  Two rounds: optimize(5); every
 * pair tested with the stored errors of the last computeActiveErrors (the last
 * LM trial, accepted or not) as chi2(e12) > th2 || chi2(e21) > th2 (a NaN keeps
 * the pair), failing pairs cleared in matches12; fewer than 10 left: return 0
 * at once with the Sim3 untouched (returned_early = 1); else optimize(n_bad > 0
 * ? 10 : 5) over the rest, the same test again (clearing only), n_in counted.
 * A correspondence exists for i when matches12[i] >= 0, valid1[i] and
 * valid2[matches12[i]] (map points that exist and are not isBad()); it reads
 * keys1[i], pos1[i], keys2[i2], pos2[i2].  The camera-frame points are
 * Rcw * X + tcw in the float arithmetic of orbx_sim3_ransac, widened.
 * All arithmetic is FP64 without contraction; DESIGN.md section 4 says which
 * parts are reproducible bit for bit.
 * Arguments are checked before any device work.  ORBX_ERR_ARG: a null
 * context, query or required pointer, n1 or n2 < 0, a match index >= n2, an
 * octave outside [0, nlevels), nlevels outside 1..16, th2 not positive and
 * finite, a non-finite initial Sim3; ORBX_ERR_UNSUPPORTED: more than 4096
 * keypoints; ORBX_ERR_CAPACITY: a per-correspondence tap with cap < n_corr.
 * Zero correspondences return ORBX_OK with n_in = 0 and returned_early = 1. */
#define ORBX_SIM3_OPT_MAX_LM 15       /* optimize(5) + optimize(10) */
#define ORBX_SIM3_OPT_MAX_TRIALS 10   /* Levenberg trials per iteration */
typedef struct {
    /* in */
    const orbx_keypoint* keys1; int n1;   /* pKF1's mvKeysUn (x, y and octave are read)        */
    const orbx_keypoint* keys2; int n2;   /* pKF2's                                            */
    int32_t* matches12;                   /* n1, in and out: >= 0 the KF2 keypoint i2 =
                                             GetIndexInKeyFrame(pKF2) of vpMatches1[i]; -1 NULL;
                                             any other negative: a non-NULL entry whose point KF2
                                             does not observe (skipped and left as it is).  Out:
                                             -1 where a check cleared the entry                */
    const float* pos1; const uint8_t* valid1;   /* n1 x 3 GetWorldPos(), n1: 1 = KF1's own map
                                                   point at i exists and is not bad             */
    const float* pos2; const uint8_t* valid2;   /* n2 x 3, n2: the matched point is not bad     */
    const float* T1w; const float* T2w;   /* 16 each: the keyframes' Tcw, row-major            */
    const float* cam1; const float* cam2; /* fx, fy, cx, cy                                    */
    const float* inv_sigma2_1;            /* nlevels: pKF1's mvInvLevelSigma2 (e12's information,
                                             src/Optimizer.cc:894)                             */
    const float* sigma2_2;                /* nlevels: pKF2's mvLevelSigma2 -- the level's sigma2,
                                             NOT its inverse: the reference calls GetSigma2 for
                                             e21 (src/Optimizer.cc:912), and so does this       */
    int nlevels;
    float R12[9], t12[3], s12;            /* in: the Sim3 as orbx_sim3_query returns it; out: the
                                             optimised one (untouched when returned_early)     */
    float th2;                            /* 10 (src/LoopClosing.cc:328)                       */
    /* out */
    int n_in;                             /* the return value of OptimizeSim3                  */
    int n_corr, n_bad;                    /* nCorrespondences; nBad of the first check         */
    int returned_early;                   /* the nCorrespondences - nBad < 10 exit             */
    double q12[4], t12d[3], s12d;         /* g2oS12 (x, y, z, w); untouched when returned_early */
    int iterations[2], trials[2], not_posdef[2];   /* per optimize(): LM iterations, trials and
                                                      LDLT failures, as orbx_pose_stats        */
    /* optional taps (may be NULL) per correspondence, cap entries each, n_corr written */
    int cap;
    int32_t* corr_index;                  /* vnIndexEdge                                       */
    float* x3dc1; float* x3dc2;           /* x 3: P3D1c, P3D2c                                 */
    double* edge_err;                     /* x 4: e12, e21 errors at round 0's first iteration */
    double* edge_J;                       /* x 28: their 2 x 7 Jacobians, row-major, e12 first */
    double* edge_chi2;                    /* 2 x cap x 2: chi2 of (e12, e21) as each check tested
                                             it (untouched where a pair was not tested)        */
    /* optional taps per LM iteration, ORBX_SIM3_OPT_MAX_LM entries each, both rounds in order */
    int n_lm;                             /* out: iterations[0] + iterations[1]                */
    double* it_est;                       /* x 8: the estimate at the iteration's start (q, t, s) */
    double* it_chi2;                      /* the robust chi2 there                             */
    double* it_H;                         /* x 28: H's lower triangle, row-major packed        */
    double* it_b;                         /* x 7                                               */
    double* it_lambda;                    /* lambda after the iteration                        */
    int32_t* it_trials;
    double* it_dx;                        /* x ORBX_SIM3_OPT_MAX_TRIALS x 7: each trial's step
                                             (zeros where the LDLT failed and past the last)   */
    double* check_est;                    /* 2 x 8: the estimate of the last trial of each round,
                                             where the tested errors were computed             */
} orbx_sim3_opt_query;

int orbx_optimize_sim3(orbx_ctx* ctx, orbx_sim3_opt_query* q);   /* one upload, one read-back */
/* Every candidate whose RANSAC returned, in one upload, one launch and one
 * read-back; results as B single calls.  The reference optimises candidate
 * after candidate until one keeps 20 (src/LoopClosing.cc:328-336); the caller
 * takes the first such in the reference's order. */
int orbx_optimize_sim3_batch(orbx_ctx* ctx, int B, orbx_sim3_opt_query* qs);
/* The same between device-resident frames: keypoints and octaves are read
 * from slot1 and slots2[k] as orbx_dev_sim3_candidates reads them; kf1 / kf2s
 * carry what does not live in a slot (mp: 1 = a good map point; sigma2 is
 * read from kf2s[k] only), inv_sigma2_1 (nlevels) is KF1's mvInvLevelSigma2.
 * out[k]: matches12 (one entry per keypoint of slot1), R12 / t12 / s12, th2,
 * cap and the tap pointers are read, the out fields written; its other in
 * fields are ignored.  Results are byte-equal to orbx_optimize_sim3_batch on
 * the slots' keypoints.  An octave outside [0, nlevels) in a slot is clamped;
 * nlevels is the extractor's (ORBX_ERR_ARG otherwise). */
int orbx_dev_optimize_sim3(orbx_ctx* ctx, int slot1, const orbx_sim3_kf* kf1, const float* inv_sigma2_1, int n,
                           const int* slots2, const orbx_sim3_kf* kf2s, orbx_sim3_opt_query* out);

/* Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:540-789), the call of
 * LoopClosing::CorrectLoop (src/LoopClosing.cc:553) after SearchAndFuse: a
 * 7-DoF pose graph over every keyframe of the map, then the Sim3 -> SE3
 * recovery of every keyframe pose and the correction of every map point.
 * g2o as the reference configures it: one VertexSim3Expmap per keyframe (the
 * loop keyframe fixed), EdgeSim3 with information I7 and error
 * (C * v0 * v1.inverse()).log(), no robust kernel, BaseBinaryEdge's central
 * differences with delta 1e-9, BlockSolver_7_3 without a Schur step over a
 * sparse Cholesky of H + lambda I, Levenberg with setUserLambdaInit(1e-16),
 * optimize(20), at most 10 trials per iteration and ORB-SLAM's stop rule.
 * The free vertices are ordered by id; a keyframe without an edge is not part
 * of the system and keeps its estimate.  A failed factorisation (a pivot that
 * is not positive and finite) rejects the trial with a zero step.
 * The factorisation is a block Cholesky in envelope storage by block row
 * (orbx_essgraph_plan): row r keeps the 7 x 7 blocks first[r]..r.
 * All arithmetic is FP64 without contraction, every sum in an order fixed by
 * the problem; two calls on the same input give the same bytes, with or
 * without taps or timing.
 * Arguments are checked before any device work and a refused call leaves every
 * caller array untouched.  ORBX_ERR_ARG: a null context, query or required
 * pointer, a negative count, n_kf < 1, an index outside its array, duplicate
 * ids, i == j on an edge, a kind other than 0 / 1, a non-finite pose or Sim3
 * or one with s <= 0.  ORBX_ERR_UNSUPPORTED: n_kf above ORBX_ESSGRAPH_MAX_KF
 * or a factor above ORBX_ESSGRAPH_MAX_FACTOR_BYTES (4096 keyframes with 16
 * edges each pass).  n_edges == 0, or no free vertex with an edge: ORBX_OK,
 * zero iterations; the recovery and the point correction still run. */
#define ORBX_ESSGRAPH_MAX_LM 20                 /* optimize(20) */
#define ORBX_ESSGRAPH_MAX_KF 16384
#define ORBX_ESSGRAPH_MAX_FACTOR_BYTES (1ll << 30)   /* n_blocks x 49 x 8 */
typedef struct {
    int64_t id;                 /* mnId: unique; orders the free vertices                */
    float Tcw[12];              /* R row-major, then t                                    */
    int32_t has_corrected;      /* CorrectedSim3.count(pKF)                               */
    int32_t has_noncorrected;   /* NonCorrectedSim3.count(pKF)                            */
    double corrected[8];        /* (x, y, z, w, tx, ty, tz, s), as q12 / t12d / s12d      */
    double noncorrected[8];
} orbx_essgraph_kf;
typedef struct {
    int32_t i, j;               /* vertex 0 = keyframe i, vertex 1 = keyframe j (indices) */
    uint8_t kind;               /* 0: loop connection, the measurement vScw[j] * vScw[i]^-1;
                                   1: normal edge, each side from noncorrected where present,
                                   else vScw                                              */
} orbx_essgraph_edge;
typedef struct {
    /* in */
    const orbx_essgraph_kf* kfs; int n_kf;   /* the caller's vpKFs order, bad keyframes left out */
    int loop_kf, cur_kf;                     /* indices; the loop keyframe is fixed              */
    const orbx_essgraph_edge* edges; int n_edges;   /* g2o insertion order                      */
    const float* pos; const int32_t* ref_kf; int n_points;   /* n x 3; the index of the keyframe
                                                of src/Optimizer.cc:765-774, -1: skipped (isBad),
                                                its output bytes left alone                     */
    /* out */
    float* Tcw_out;                          /* n_kf x 12                                        */
    float* pos_out;                          /* n_points x 3 (may be NULL when n_points == 0)    */
    double* est_out;                         /* optional, n_kf x 8: the optimised Sim3           */
    int iterations, trials, not_posdef;
    double chi2_first, chi2_last, lambda_last;
    int n_free;                              /* vertices of the system                           */
    long long n_blocks;                      /* 7 x 7 blocks the factorisation stores            */
    int max_row_blocks;
    /* optional taps (may be NULL) per edge at the first iteration */
    double* edge_meas;                       /* x 8                                              */
    double* edge_err;                        /* x 7                                              */
    double* edge_J;                          /* x 98: Ji then Jj, 7 x 7 row-major, zeros for a fixed side */
    /* optional taps per LM iteration, ORBX_ESSGRAPH_MAX_LM entries each */
    double* it_chi2;
    double* it_lambda;                       /* lambda after the iteration                       */
    int32_t* it_trials;
    double* it_est;                          /* x n_kf x 8: every estimate at the iteration's start */
    double* it_b;                            /* x 7 n_free                                       */
    double* it_dx;                           /* x 7 n_free: the last trial's step                */
    double* it_Hdiag;                        /* x n_free x 28: the packed lower triangle of each
                                                diagonal block, before lambda                   */
} orbx_essgraph_query;

int orbx_optimize_essential_graph(orbx_ctx* ctx, orbx_essgraph_query* q);   /* one upload, one read-back */

/* The symbolic part of that factorisation, on the host (no device is touched):
 * the free vertices are the keyframes other than `fixed` (an index, or -1)
 * that have an edge, in id order; free_index[k] (n_kf) is keyframe k's place
 * in it or -1; first[r] (n_kf entries, n_free written) is the smallest free
 * index row r is connected to, or r; row r stores the blocks first[r]..r at
 * row_off[r] (n_kf + 1 entries, n_free + 1 written).  Output pointers may be
 * NULL.  ORBX_ERR_ARG as orbx_optimize_essential_graph checks ids and edges. */
int orbx_essgraph_plan(int n_kf, const int64_t* ids, int fixed, int n_edges, const orbx_essgraph_edge* edges,
                       int32_t* free_index, int32_t* first, int64_t* row_off, int* n_free, long long* n_blocks,
                       int* max_row_blocks);

/* PnPsolver (src/PnPsolver.cc): EPnP inside a RANSAC over the map-point
 * matches of a frame, the step of Tracking::Relocalisation
 * (src/Tracking.cc:921-947) between SearchByBoW and PoseOptimization.  One
 * call is one PnPsolver::iterate(n_iter, ...) (:137-230) of a solver built by
 * the constructor (:39-82) and SetRansacParameters (:93-129): the
 * correspondences compacted in i order, then every iteration the call can run
 * at once -- its minimal set from the caller's rand() values (four per
 * iteration; the removal writes at the drawn value, :171), compute_pose on
 * four points and CheckInliers -- Refine (:232-277) of the incoming best set
 * and of every strict record holder among the iterations with count >=
 * ransac_min_inliers, and the replay of the loop's sequential bookkeeping.
 * The loop's condition is an or (:154): a call runs max(n_iter,
 * ransac_max_its - iter_done) iterations unless a Refine returns first.
 * EPnP is FP64 and follows the reference operation by operation (never
 * contracted); CheckInliers' mixed float / double expressions follow
 * orbx_set_fp_contract; the five places that go through OpenCV are defined
 * in DESIGN.md section 4.
 * The caller continues a solver by passing the state fields back: iter_done,
 * best_inliers, best_mask and best_Tcw are read on entry and written at
 * return, with the draws that follow the iters_run * 4 consumed ones.
 * Arguments are checked before any device work.  ORBX_ERR_ARG: a null
 * context, query or required pointer, n_iter < 1, n_draws outside
 * [max(n_iter, max_iterations - iter_done), 1024], a draw < 0, min_inliers < 1,
 * max_iterations < 1, iter_done or best_inliers < 0, a probability outside
 * (0,1), an epsilon outside [0,1] or th2 not positive and finite, nlevels
 * outside 1..16, an octave outside [0, nlevels), a level sigma2 that is
 * negative or not finite; ORBX_ERR_UNSUPPORTED: min_set other than 4, more
 * than 4096 keypoints; ORBX_ERR_CAPACITY: cap < n.  N < ransac_min_inliers
 * returns ORBX_OK with no_more = 1, found = 0 and no iteration run
 * (:145-149). */
#define ORBX_PNP_DEC 135   /* doubles of decomposition taps per hypothesis */
#define ORBX_PNP_REC 232   /* doubles of one hypothesis record             */
typedef struct {
    /* in */
    const orbx_keypoint* keys; int n;     /* the frame's mvKeysUn (x, y and octave are read)   */
    const float* pos; const uint8_t* valid;   /* n x 3 GetWorldPos() of vpMapPointMatches[i];
                                                 n: 0 = NULL or isBad()                         */
    const float* cam;                     /* fx, fy, cx, cy                                    */
    const float* sigma2; int nlevels;     /* mvLevelSigma2                                     */
    double probability; int min_inliers; int max_iterations; int min_set;   /* 0.99, 8, 300, 4 */
    float epsilon; float th2;             /* 0.4, 5.991 (Relocalisation: 0.99,10,300,4,0.5,5.991) */
    /* iterate state (in and out) */
    int iter_done;                        /* mnIterations                                      */
    int best_inliers;                     /* mnBestInliers                                     */
    uint8_t* best_mask;                   /* cap >= n: mvbBestInliers by keypoint index        */
    float best_Tcw[16];                   /* mBestTcw                                          */
    /* draws */
    int n_iter;                           /* iterate's nIterations                             */
    int n_draws; const int32_t* draws;    /* n_draws x 4 successive rand() values              */
    /* out */
    int N;                                /* correspondences                                   */
    int ransac_min_inliers;               /* mRansacMinInliers after SetRansacParameters       */
    int ransac_max_its;                   /* mRansacMaxIts (0 when N < ransac_min_inliers)     */
    int iters_run;                        /* iterations executed by this call                  */
    int no_more;                          /* bNoMore                                           */
    int found, found_iter;                /* a non-empty return; the iteration whose Refine
                                             returned, -1 for the mBest* exit (:213-227)       */
    int n_inliers;                        /* nInliers (0 when !found)                          */
    int refined;                          /* 1: the return came from Refine                    */
    float Tcw[16];                        /* the returned pose (untouched when !found)         */
    uint8_t* inliers; int cap;            /* vbInliers by keypoint index (n written)           */
    int n_records;                        /* strict record holders among the call's iterations */
    int best_slot;                        /* the refit that belongs to the best state at
                                             return: 0 the incoming one, k the k-th record     */
    /* optional taps per correspondence (cap entries each, N written) */
    float* p2d; float* p3d; float* max_err; int32_t* kp_index;   /* x 2, x 3, mvMaxError, mvKeyPointIndices */
    /* optional taps per iteration (n_draws entries each) */
    int32_t* sets;                        /* x 4: indices into the correspondences             */
    double* rec;                          /* x ORBX_PNP_REC, FP64: [0,135) the decompositions
                                             (dc 3, UCt 9, CC_inv 9, rows 8..11 of Ut 48, the
                                             three cvSolve results 4 + 3 + 5, U and V of ABt per
                                             beta set 3 x 18), L_6x10 60, rho 6, the betas after
                                             gauss_newton 3 x 4, R 9, t 3, rep_errors 3, the
                                             chosen set (1..3), the number of points           */
    int32_t* count;                       /* mnInliersi                                        */
    /* optional taps per refit (n_draws + 1 entries: the incoming state, then each record) */
    double* refit_rec; int32_t* refit_count; int32_t* record_iter;
} orbx_pnp_query;

int orbx_pnp_ransac(orbx_ctx* ctx, orbx_pnp_query* q);   /* one upload, one read-back */
/* Relocalisation's candidates in one upload, one launch set and one
 * read-back; results as B single calls. */
int orbx_pnp_ransac_batch(orbx_ctx* ctx, int B, orbx_pnp_query* qs);

/* Relocalisation's loop over n candidate keyframes with the frame resident in
 * `slot` (after orbx_dev_compute_bow): SearchByBoW(pKF, F) as
 * orbx_dev_search_by_bow queues it, and on the match vectors where the search
 * left them a solver per candidate: the correspondence at frame keypoint i is
 * the map point of keyframe keypoint matches_f[k][i] (KFs[k].mp must read 1
 * there), its position pos[k] (KFs[k].n x 3).  cam, sigma2 and nlevels are
 * the frame's.  A candidate with n_matches[k] < min_matches (15,
 * Tracking.cc:914) gets discarded[k] = 1 and runs no RANSAC (N = 0, found =
 * 0, no_more = 0).  The RANSAC parameters, n_iter, n_draws and the iterate
 * state are read from out[k] (its keys, pos, valid, cam and sigma2 are
 * ignored), draws from out[k].draws; out[k].inliers / best_mask hold cap >=
 * nfeatures entries.  One synchronisation and one read-back.  Results as
 * orbx_dev_search_by_bow followed by orbx_pnp_ransac_batch on the read-back
 * matches.  A match whose index or octave is out of range is dropped. */
int orbx_dev_pnp_candidates(orbx_ctx* ctx, int slot, int n, const orbx_bow_view* KFs, const float* const* pos,
                            const float* cam, const float* sigma2, int nlevels, float nnratio, int check_ori,
                            int min_matches, int32_t* const* matches_f, int cap, int* n_matches, int* discarded,
                            orbx_pnp_query* out);

/* KeyFrameDatabase (src/KeyFrameDatabase.cc): the BowVectors of the map's
 * keyframes in HBM, and DetectRelocalisationCandidates (:198-308) /
 * DetectLoopCandidates (:75-196) as one call per query, the latter with
 * DetectLoop's reference score (src/LoopClosing.cc:119-139) in front.  The
 * result is the reference's vector: the same keyframes in the same order.
 *
 * Members are named by the caller's ids in [0, capacity) (KeyFrame::mnId as it
 * is; nothing is renumbered).  capacity is at most ORBX_KFDB_MAX_MEMBERS and
 * max_words (the longest BowVector of a member or a query) at most
 * ORBX_KFDB_MAX_WORDS; above either orbx_kfdb_create returns
 * ORBX_ERR_UNSUPPORTED (the select kernel orders the sharing list in one
 * workgroup's LDS; the scan kernel keeps the query there).  A database
 * belongs to the device of the context it was created with and is used with
 * contexts of that device, one thread at a time.
 *
 * The inverted file's list order is kept as an add counter per database:
 * lKFsSharingWords is ordered by (smallest common word, add order), erase
 * keeps the others' order and an id added again goes to the back.  The counter
 * holds 2^32 - 1 adds between two orbx_kfdb_clear calls (ORBX_ERR_UNSUPPORTED
 * after).
 *
 * KeyFrame::mRelocScore is kept per member across relocalisation queries, as
 * the reference's field is: written for the members that pass a query's word
 * gate, read for a neighbour that shares a word but failed it.  The reference
 * never initialises the field (src/KeyFrame.cc:33), so its first read there
 * is indeterminate; here it is 0.0f from orbx_kfdb_add / _add_slot on.  The
 * loop query's mLoopScore is only ever read after this query wrote it, so it
 * keeps no state. */
#define ORBX_KFDB_MAX_MEMBERS 8192
#define ORBX_KFDB_MAX_WORDS   4096
#define ORBX_KFDB_NEIGHBOURS  10     /* GetBestCovisibilityKeyFrames(10) */
#define ORBX_KFDB_RELOC 0
#define ORBX_KFDB_LOOP  1
typedef struct orbx_kfdb orbx_kfdb;
int orbx_kfdb_create(orbx_ctx* ctx, int capacity, int max_words, orbx_kfdb** out);
void orbx_kfdb_destroy(orbx_kfdb* db);
/* KeyFrameDatabase::clear: no members, every neighbour row and score reset. */
int orbx_kfdb_clear(orbx_ctx* ctx, orbx_kfdb* db);
int orbx_kfdb_size(const orbx_kfdb* db);   /* members; ORBX_ERR_ARG for NULL */
/* KeyFrameDatabase::add from host arrays: words strictly ascending (a
 * BowVector's iteration order), values finite.  ORBX_ERR_ARG: id outside
 * [0, capacity) or in use, unordered words, a value that is not finite;
 * ORBX_ERR_CAPACITY: n_words > max_words.  The arrays are free at return. */
int orbx_kfdb_add(orbx_ctx* ctx, orbx_kfdb* db, int id, int n_words, const uint32_t* words, const double* values);
/* add of the BowVector orbx_dev_compute_bow left in `slot`: a device-to-device
 * copy queued on the context's stream, the word count read on the device, no
 * synchronisation.  ORBX_ERR_ARG: a slot without valid BoW; ORBX_ERR_CAPACITY:
 * max_words below the context's nfeatures (the most words a slot can hold). */
int orbx_kfdb_add_slot(orbx_ctx* ctx, orbx_kfdb* db, int id, int slot);
/* KeyFrameDatabase::erase: frees the id, clears the member's neighbour row
 * and its relocalisation score.  ORBX_ERR_ARG: not a member. */
int orbx_kfdb_erase(orbx_ctx* ctx, orbx_kfdb* db, int id);
/* The rows GetBestCovisibilityKeyFrames(10) returns for members ids[0, n)
 * (call it where KeyFrame::UpdateBestCovisibles runs): neigh is n x 10 member
 * ids in that order, padded with -1; stored in HBM.  An entry that does not
 * name a member when a query runs is skipped by that query.  ORBX_ERR_ARG:
 * an id of ids that is not a member. */
int orbx_kfdb_set_neighbours(orbx_ctx* ctx, orbx_kfdb* db, int n, const int32_t* ids, const int32_t* neigh);

typedef struct {
    /* in */
    int mode;                             /* ORBX_KFDB_RELOC or ORBX_KFDB_LOOP                  */
    int slot;                             /* >= 0: the query is the BowVector of this slot, read
                                             in HBM (max_words >= nfeatures, as for add_slot);
                                             -1: the host arrays below                          */
    int n_words; const uint32_t* words; const double* values;   /* as for orbx_kfdb_add        */
    /* loop only (ignored for relocalisation) */
    float min_score;                      /* DetectLoop's start value (1), or DetectLoopCandidates'
                                             minScore itself with n_ref = 0                     */
    int n_ref; const int32_t* ref;        /* GetVectorCovisibleKeyFrames: min_score_used is the
                                             minimum of min_score and the scores against these  */
    int n_exclude; const int32_t* exclude;   /* GetConnectedKeyFrames: never listed             */
    /* out */
    int32_t* candidates; int cap;         /* the returned vector, in order                      */
    int n_candidates;                     /* its size (ORBX_ERR_CAPACITY when above cap; cap
                                             entries are written then)                          */
    float min_score_used;                 /* loop: minScore; relocalisation: 0                  */
    int max_common_words;                 /* maxCommonWords (0: nothing shares a word)          */
    int n_sharing;                        /* lKFsSharingWords.size()                            */
    int n_scored;                         /* nscores                                            */
    /* optional taps per member id, capacity entries each (NULL: not read back) */
    int32_t* tap_words;                   /* mnRelocWords / mnLoopWords of a listed member, else 0 */
    float* tap_score;                     /* relocalisation: mRelocScore after the query; loop:
                                             mLoopScore of a member that passed the gate, else 0 */
    float* tap_acc; int32_t* tap_best;    /* accScore and pBestKF of a member of lScoreAndMatch,
                                             else 0 and -1                                      */
    int32_t* tap_pos;                     /* position in lKFsSharingWords, else -1              */
} orbx_kfdb_query_args;

/* One query: one upload (the query's arrays and the two lists; the lists alone
 * for a slot query), the scan and select kernels, one read-back (the header
 * and cap candidates; the taps only when asked for).  ref and exclude ids lie
 * in [0, capacity) (ORBX_ERR_ARG otherwise); one that is not a member is
 * skipped, as DetectLoop skips a bad keyframe.  An empty database, an empty
 * query and a query that shares no word return ORBX_OK with n_candidates = 0.
 * ORBX_ERR_ARG: a null pointer, another mode, a slot without valid BoW, host
 * words out of order, cap < 0; ORBX_ERR_CAPACITY: n_words > max_words, a slot
 * query with max_words below nfeatures, n_candidates > cap. */
int orbx_kfdb_query(orbx_ctx* ctx, orbx_kfdb* db, orbx_kfdb_query_args* q);
/* mpVoc->score(query, member ids[k]) as the float the reference stores, for n
 * named members (DetectLoop's loop on its own): the scan kernel alone.  The
 * query is given as in orbx_kfdb_query (slot >= 0, or -1 and host arrays).
 * ORBX_ERR_ARG: an id that is not a member. */
int orbx_kfdb_score(orbx_ctx* ctx, orbx_kfdb* db, int slot, int n_words, const uint32_t* words, const double* values,
                    int n, const int32_t* ids, float* scores);

/* The covisibility graph in HBM: the keyframe -> map-point table
 * (KeyFrame::mvpMapPoints of every keyframe) and the connection weights
 * (mConnectedKeyFrameWeights), with KeyFrame::UpdateConnections
 * (src/KeyFrame.cc:332-421), the covisibility reads (:162-211) and
 * Tracking::UpdateReferenceKeyFrames + UpdateReferencePoints
 * (src/Tracking.cc:764-865) on top of them.  Integer work throughout: every
 * list comes back as the reference builds it, entry for entry.
 *
 * Ids.  Keyframes are named by mnId in [0, kf_capacity), kf_capacity <=
 * ORBX_COVIS_MAX_KEYFRAMES; map points by mnId in [0, mp_capacity),
 * mp_capacity <= ORBX_COVIS_MAX_POINTS; a row holds at most max_keypoints <=
 * ORBX_COVIS_MAX_KEYPOINTS entries.  Above a limit orbx_covis_create returns
 * ORBX_ERR_UNSUPPORTED.  An id is never reused: adding a keyframe id that was
 * erased is ORBX_ERR_ARG (until orbx_covis_clear).
 *
 * Order keys.  The reference iterates std::map<KeyFrame*, ...> and sorts
 * pair<int, KeyFrame*>, so pointer values decide the order of its lists.
 * Every keyframe is added with a 64-bit key that stands for that value (the
 * adapter passes (uint64_t)(uintptr_t)pKF), distinct among all keyframes ever
 * added.
 *
 * Observations.  The observation set of point p is, by definition, the
 * members whose row holds p.  That equals MapPoint::mObservations wherever
 * KeyFrame::AddMapPoint / MapPoint::AddObservation and EraseMapPointMatch /
 * EraseObservation have been applied in pairs, which is the case at every
 * call site of the three operations.  A keyframe is therefore added where
 * LocalMapping::ProcessNewKeyFrame has added its observations
 * (src/LocalMapping.cc:130-160), not where Tracking constructs it.  A point
 * stands at most once in a row (mObservations holds one index per keyframe).
 * MapPoint::EraseObservation turns a point bad when two observations or
 * fewer remain; that is a SetBadFlag, mirrored with orbx_covis_erase_points
 * (orbx_covis_cull_keyframes applies the rule itself for the keyframes it
 * culls).
 *
 * Erased points (MapPoint::isBad()).  An erased id in an input row or in a
 * frame is no error: it is skipped as the reference skips a bad point.
 *
 * Connection state of member i: the weights W[i][j] > 0, a flag filtered_i and
 * a threshold th_i.  The ordered list (mvpOrderedConnectedKeyFrames /
 * mvOrderedWeights) is a function of these: the entries of row i when not
 * filtered; when filtered those with weight >= th_i, or, if none passes, the
 * single entry of largest weight (the smallest key among equals); sorted
 * descending by (weight, key): among equal weights the larger key first.
 *
 * Every edit is applied to a host shadow (where it is checked) and mirrored
 * to HBM on the context's stream.  An object belongs to the device of the
 * context it was created with; one thread at a time. */
#define ORBX_COVIS_MAX_KEYFRAMES 8192
#define ORBX_COVIS_MAX_KEYPOINTS 65535
#define ORBX_COVIS_MAX_POINTS    (1 << 27)
#define ORBX_COVIS_ORDERED 0
#define ORBX_COVIS_ALL     1
typedef struct orbx_covis orbx_covis;
int orbx_covis_create(orbx_ctx* ctx, int kf_capacity, int mp_capacity, int max_keypoints, orbx_covis** out);
void orbx_covis_destroy(orbx_covis* m);
/* No keyframes, no erased points, every id and key free again. */
int orbx_covis_clear(orbx_ctx* ctx, orbx_covis* m);
int orbx_covis_size(const orbx_covis* m);   /* member keyframes; ORBX_ERR_ARG for NULL */
/* A keyframe with its row mvpMapPoints: n <= max_keypoints entries, a point id
 * or -1 each.  ORBX_ERR_ARG: id out of range, in use or erased; a key used
 * before; n or an entry out of range; a point twice in the row. */
int orbx_covis_add_keyframe(orbx_ctx* ctx, orbx_covis* m, int id, uint64_t key, int n, const int32_t* mp);
/* Scattered writes to member id's row, in order: row[idx[k]] = mp[k]; -1 is
 * EraseMapPointMatch, a point id AddMapPoint / ReplaceMapPointMatch.  All or
 * none: ORBX_ERR_ARG (and no change) for an index outside the row, a point out
 * of range or a point that would stand twice in the row. */
int orbx_covis_set_matches(orbx_ctx* ctx, orbx_covis* m, int id, int n_edits, const int32_t* idx, const int32_t* mp);
/* MapPoint::SetBadFlag, and Replace's old point: marks the points erased and
 * clears them from every row.  ORBX_ERR_ARG: an id out of range. */
int orbx_covis_erase_points(orbx_ctx* ctx, orbx_covis* m, int n, const int32_t* ids);
/* The connection part of KeyFrame::SetBadFlag (src/KeyFrame.cc:510-521): for
 * every j in row id of W, an existing W[j][id] is erased and filtered_j
 * cleared (EraseConnection -> UpdateBestCovisibles); then row id of W and the
 * keyframe's table row go.  A W[j][id] without a W[id][j] stays, as the
 * reference's dangling KeyFrame* does; the reads report it as it stands.  The
 * spanning tree stays with the caller, which reads what it needs through
 * orbx_covis_connections before this call.  ORBX_ERR_ARG: not a member. */
int orbx_covis_erase_keyframe(orbx_ctx* ctx, orbx_covis* m, int id);
/* KeyFrame::UpdateConnections for members ids[0, n), in that order, with the
 * reference's threshold th (15).  For i = ids[k]: counter[j] = the entries of
 * row i that are not -1, not erased and in row j (j != i a member).  All zero:
 * nothing changes, updated[k] = 0, front[k] = -1.  Otherwise row i of W
 * becomes the non-zero counts (those below th included), filtered_i = 1, th_i
 * = th; AddConnection(j <- i) runs for every j with counter[j] >= th, or for
 * the single fallback keyframe: an unchanged W[j][i] leaves j as it is, a
 * changed or new one is written and clears filtered_j.  updated[k] = 1 and
 * front[k] = the head of i's ordered list (mpParent under mbFirstConnection).
 * updated / front hold n entries.  ORBX_ERR_ARG: an id that is not a member,
 * th < 1. */
int orbx_covis_update_connections(orbx_ctx* ctx, orbx_covis* m, int n, const int32_t* ids, int th, int32_t* updated,
                                  int32_t* front);
/* which = ORBX_COVIS_ORDERED: the ordered list of member id and its weights
 * (GetVectorCovisibleKeyFrames; its first N entries are
 * GetBestCovisibilityKeyFrames(N)); ORBX_COVIS_ALL: every entry of row id in
 * ascending key order (GetConnectedKeyFrames with GetWeight).  Entries that
 * name an erased keyframe are reported (the reference's callers test
 * isBad()).  *n = the list's length; ORBX_ERR_CAPACITY when it exceeds cap
 * (cap entries are written then). */
int orbx_covis_connections(orbx_ctx* ctx, orbx_covis* m, int id, int which, int32_t* kfs, int32_t* weights, int cap,
                           int* n);

typedef struct {
    /* in */
    int n; const int32_t* frame_mp;       /* mCurrentFrame.mvpMapPoints: ids or -1, n <= max_keypoints;
                                             a point may stand twice and then votes twice           */
    /* out */
    uint8_t* frame_erased;                /* [n] 1 where the point is erased: the caller NULLs it
                                             (src/Tracking.cc:805-808); NULL: not wanted            */
    int32_t* local_kf; int kf_cap;        /* mvpLocalKeyFrames                                      */
    int n_local_kf;                       /* its size                                               */
    int n_voters;                         /* its size before the neighbour pass                     */
    int ref_kf;                           /* mpReferenceKF (pKFmax), or -1                          */
    int32_t* local_mp; int mp_cap;        /* mvpLocalMapPoints                                      */
    int n_local_mp;                       /* its size                                               */
} orbx_covis_reference_args;
/* Tracking::UpdateReferenceKeyFrames + UpdateReferencePoints for one frame.
 * Votes: every frame entry that is a point and not erased votes for the
 * members whose row holds it.  The voters in ascending key order open
 * local_kf; ref_kf is the first strict maximum in that order.  The neighbour
 * pass visits the voters in that order, stops before a voter once the list
 * holds more than 80 keyframes, and appends the first of the voter's best 10
 * (erased keyframes take places among the 10) that is a member and not yet
 * listed.  local_mp: the rows of the local keyframes in list and index
 * order, every point that is not erased once, at its first place.  Both lists
 * also stay in buffers of the object in HBM.  ORBX_ERR_ARG: n or an entry out
 * of range, cap < 0; ORBX_ERR_CAPACITY with the three counts set when a list
 * exceeds its capacity (the capacity's worth of entries is written). */
int orbx_covis_update_reference(orbx_ctx* ctx, orbx_covis* m, orbx_covis_reference_args* q);

/* LocalMapping's two culling walks on the table (src/LocalMapping.cc:190-218,
 * :539-593).
 *
 * mvKeysUn[i].octave of member id, n = the row length given at
 * orbx_covis_add_keyframe.  orbx_covis_cull_keyframes needs them of every
 * member.  ORBX_ERR_ARG: not a member, another n, a null pointer with n > 0. */
int orbx_covis_set_octaves(orbx_ctx* ctx, orbx_covis* m, int id, int n, const uint8_t* octave);

typedef struct {
    /* in */
    int cur;                              /* mpCurrentKeyFrame, a member: the candidates are its ordered
                                             list (GetVectorCovisibleKeyFrames) as the call finds it, taken
                                             on the device; -1: the caller's list cand[0, n_cand)          */
    int n_keep; const int32_t* keep;      /* the keyframes with mbNotErase set; may be empty               */
    int max_culls;                        /* 0: no limit; else the call stops right after that many culls  */
    int cand_cap;                         /* entries of cand, n_mps, n_redundant and decision              */
    /* in (cur == -1) / out */
    int32_t* cand; int n_cand;            /* vpLocalKeyFrames                                              */
    /* out */
    int n_done;                           /* candidates processed                                          */
    int32_t* n_mps;                       /* [n_done] nMPs                                                 */
    int32_t* n_redundant;                 /* [n_done] nRedundantObservations                               */
    int32_t* decision;                    /* [n_done] -1: keyframe 0 or no member, skipped; 0: stays;
                                             1: culled; 2: redundant but kept (mbToBeErased)               */
    int32_t* bad_points; int bad_cap;     /* the points that a cull left with two observers or fewer, by
                                             culled keyframe in candidate order, ascending row index within */
    int n_bad;                            /* its size                                                      */
} orbx_covis_cull_args;
/* LocalMapping::KeyFrameCulling.  Candidate c at place k is judged against the
 * state (members, rows, erased points, connections) as the candidates before
 * it left it.  c == 0 or no member: decision -1, nothing changes.  Otherwise
 * nMPs = the entries of row c that are a point and not erased; such an entry
 * (idx, p) with o = octave_c[idx] is redundant when at least three members
 * j != c hold p at an index idx_j with octave_j[idx_j] <= o + 1.  With
 * (double)nRedundant > 0.9 * (double)nMPs false the decision is 0; true with c
 * in keep it is 2 and nothing changes; true otherwise it is 1 and the graph
 * part of KeyFrame::SetBadFlag runs: the connection part exactly as
 * orbx_covis_erase_keyframe, row c goes, and MapPoint::EraseObservation for
 * every point of the row: a point, not erased, that two members or fewer still
 * hold becomes erased and is cleared from every row, as orbx_covis_erase_points
 * does it, and is appended to bad_points.  The spanning tree stays with the
 * caller, which reads the children's lists right after one cull: call with
 * max_culls = 1, repair the tree, resume with cur = -1 and cand + n_done.  A
 * resumed sequence leaves the state and the decisions of one unlimited call.
 * ORBX_ERR_ARG (no change): cur no member (or below -1), a listed or kept id
 * outside [0, kf_capacity), n_cand above kf_capacity, a member whose octaves
 * were never set, max_culls or a count or capacity below 0, a null pointer.
 * ORBX_ERR_CAPACITY (no change to the graph, n_cand, n_done and n_bad set, the
 * capacities' worth of entries written): n_cand > cand_cap or n_bad > bad_cap;
 * n_cand <= kf_capacity, n_bad <= the sum of the culled rows' lengths. */
int orbx_covis_cull_keyframes(orbx_ctx* ctx, orbx_covis* m, orbx_covis_cull_args* q);
/* LocalMapping::MapPointCulling over mlpRecentAddedMapPoints = ids[0, n), each
 * id once, with mnFound, mnVisible and mnFirstKFid of each and cur_kf =
 * mpCurrentKeyFrame->mnId.  action[k], by the reference's if-chain: 1 the point
 * is erased already (drop it from the list); 2 (float)found / (float)visible <
 * 0.25f in FP32 (visible == 0 gives inf or NaN: false): SetBadFlag and drop; 3
 * cur_kf - first_kf >= 2 and two observers (members whose row holds the point)
 * or fewer: SetBadFlag and drop; 4 cur_kf - first_kf >= 3: drop; 0 keep.  The
 * points of actions 2 and 3 are erased as orbx_covis_erase_points erases them.
 * ORBX_ERR_ARG (no change): an id out of range or listed twice, found or
 * visible below 0, first_kf > cur_kf or below 0, n < 0, a null pointer with
 * n > 0. */
int orbx_covis_cull_points(orbx_ctx* ctx, orbx_covis* m, int cur_kf, int n, const int32_t* ids, const int32_t* found,
                           const int32_t* visible, const int32_t* first_kf, int32_t* action);

/* ------------------------------------------------------------------------ */
/* C. Local bundle adjustment                                                */
/* ------------------------------------------------------------------------ */

/* SoA local-BA problem (Optimizer::LocalBundleAdjustment, src/Optimizer.cc:
 * 287-536).  Poses are SE3Quat (g2o se3quat.h) as unit quaternion (x,y,z,w)
 * + translation; ids are the g2o vertex ids (KF mnId; points mnId+maxKFid+1)
 * which fix the Hessian ordering (sparse_optimizer.cpp:166-190, 482-487).
 * Edges are EdgeSE3ProjectXYZ in insertion order (points in local-list order,
 * observations in the caller's map<KeyFrame*,size_t> order).  huber_delta
 * and chi2_threshold are per problem: in a batch (orbx_lba_solve_batch,
 * orbx_lba_stage) every problem is solved and gated with its own pair. */
typedef struct {
    int n_poses, n_points, n_edges;
    double* pose_q;             /* [n_poses][4] x,y,z,w   (in/out)           */
    double* pose_t;             /* [n_poses][3]           (in/out)           */
    const uint8_t* pose_fixed;  /* [n_poses]                                  */
    const int64_t* pose_id;     /* [n_poses] g2o vertex id                    */
    const double* pose_cam;     /* [n_poses][4] fx, fy, cx, cy                */
    double* points;             /* [n_points][3]          (in/out)           */
    const int64_t* point_id;    /* [n_points]                                 */
    const int32_t* point_nobs;  /* [n_points] MapPoint::Observations() at call*/
    const int32_t* edge_point;  /* [n_edges] index into points                */
    const int32_t* edge_pose;   /* [n_edges] index into poses                 */
    const double* edge_obs;     /* [n_edges][2] undistorted keypoint          */
    const double* edge_inv_sigma2; /* [n_edges] information = I * invSigma2   */
    double huber_delta;         /* sqrt(5.991) as float, widened              */
    double chi2_threshold;      /* 5.991                                      */
} orbx_ba_problem;

typedef struct {
    int iterations[2];          /* LM iterations executed per optimize() call */
    int levenberg_trials[2];    /* inner LM trials summed                     */
    double chi2_initial[2];     /* robust chi2 at the first linearisation     */
    double chi2_final[2];       /* robust chi2 of the accepted state          */
    int n_outliers[2];          /* edges erased by each outlier pass          */
    int not_posdef;             /* Cholesky failures (step rejected)          */
} orbx_ba_stats;

/* Runs optimize(iters0), the first outlier pass (edge erased and removed from
 * the graph), optimize(iters1) and the second outlier pass.  edge_status
 * (out, n_edges): 0 inlier, 1 erased in pass 1, 2 erased in pass 2.
 * point_bad (out, n_points): MapPoint became bad through EraseObservation.
 * abort: polled between LM iterations (mbAbortBA; may be NULL).  g2o also
 * tests its stop flag between the trials of an iteration (levenberg.cpp:149);
 * here an iteration that has started runs its trials to the end, so a flag
 * raised mid-iteration stops the solve at the same iteration boundary but
 * possibly after more trials.
 * One problem runs over several workgroups when it qualifies
 * (orbx_lba_set_workgroups), with the same result bits. */
int orbx_lba_solve(orbx_ctx* ctx, orbx_ba_problem* p, int iters0, int iters1,
                   const volatile uint8_t* abort, uint8_t* edge_status,
                   uint8_t* point_bad, orbx_ba_stats* stats);

/* Workgroups that share one problem (orbx_lba_solve, and batches of one):
 * 0 (default) = automatic (one per 32 points, at most 64, when the reduced
 * system fits a workgroup's LDS); 1 = one workgroup, as in a batch; n > 1 =
 * n workgroups.  Every setting gives the same bits (k_lba_split sums in the
 * single-workgroup kernel's order); more workgroups cut the latency of the
 * call LocalMapping makes once per keyframe (src/LocalMapping.cc:83).
 * The workgroups of one problem meet at grid barriers, so they must all be
 * resident at once: the count is capped at what the device holds of that
 * kernel (occupancy x CUs: a partitioned device, or a setting of 256, gets
 * fewer), and a solve whose barrier still times out (another context's
 * kernels holding the CUs) is run again on one workgroup -- same bits,
 * longer call.  (A cooperative launch, available through
 * orbx_debug_lba_split, gives the same bits but measured to delay other
 * contexts' calls beside it.) */
int orbx_lba_set_workgroups(orbx_ctx* ctx, int n);
int orbx_lba_get_workgroups(const orbx_ctx* ctx);
/* Workgroups the last local-BA launch of ctx ran with (after the cap and any
 * one-workgroup re-run). */
int orbx_lba_last_workgroups(const orbx_ctx* ctx);
/* Test hooks of that residency handling (fail: the next n split launches
 * see a barrier timeout; fallback 0: no re-run, ORBX_ERR_HIP with the
 * caller's arrays untouched; cap > 0: capacity capped; coop -1 / 0 / 1:
 * the device's choice / plain (default) / cooperative launch; arguments
 * below those ranges leave the setting unchanged). */
int orbx_debug_lba_split(orbx_ctx* ctx, int fail, int fallback, int cap, int coop);

/* Batched throughput form: P independent problems, one workgroup each.
 * aborts: NULL, or P flags (entries may be NULL), each polled between LM
 * iterations like orbx_lba_solve's: problem i stops its optimize() calls
 * when *aborts[i] is set (its own LocalMapping's mbAbortBA,
 * src/LocalMapping.cc:83, :125), the others continue.  With flags each
 * iteration is a launch and the call waits for it to poll; without flags
 * each optimize() pass is one launch of all its iterations and nothing
 * waits.  Results are the same bits either way. */
int orbx_lba_solve_batch(orbx_ctx* ctx, int P, orbx_ba_problem* problems,
                         int iters0, int iters1, const volatile uint8_t* const* aborts,
                         uint8_t* const* edge_status, uint8_t* const* point_bad,
                         orbx_ba_stats* stats);
/* Device-resident form of the batch (bench/tests; the pose API's shape):
 * stage P problems in HBM once (validated as orbx_lba_solve_batch does),
 * run both optimize() passes from the staged state any number of times
 * (asynchronous, on the context stream; kernel timers "lba_iter" /
 * "lba_outliers"), fetch the last run's poses, points, flags and statistics
 * into problems laid out like the staged ones (ORBX_ERR_ARG before a run or
 * on a size mismatch).  orbx_lba_run's aborts are orbx_lba_solve_batch's
 * (NULL: asynchronous; with flags the call returns when the run is done). */
int orbx_lba_stage(orbx_ctx* ctx, int P, const orbx_ba_problem* problems);
int orbx_lba_run(orbx_ctx* ctx, int iters0, int iters1, const volatile uint8_t* const* aborts);
int orbx_lba_fetch(orbx_ctx* ctx, orbx_ba_problem* problems, uint8_t* const* edge_status,
                   uint8_t* const* point_bad, orbx_ba_stats* stats);

/* ------------------------------------------------------------------------ */
/* D. Motion-only pose optimisation                   */
/* ------------------------------------------------------------------------ */

/* One Frame as Optimizer::PoseOptimization(Frame*) reads and writes it
 * (src/Optimizer.cc:154-285).  Keypoints with a map point become
 * EdgeSE3ProjectXYZ edges to fixed points (information = I *
 * mvInvLevelSigma2[octave], Huber delta sqrt(5.991)); four robust rounds
 * (chi2 9.210 / 7.378 / 5.991 / 5.991, LM iterations 10 / 10 / 7 / 5)
 * classify outliers. */
typedef struct {
    int n;                           /* N = mvpMapPoints.size() (= keypoints)    */
    const float* kp_un;              /* [n][2] mvKeysUn[i].pt                    */
    const int32_t* octave;           /* [n] mvKeysUn[i].octave                   */
    const float* inv_level_sigma2;   /* [nlevels] mvInvLevelSigma2               */
    int nlevels;
    const uint8_t* has_mp;           /* [n] mvpMapPoints[i] != NULL              */
    const float* mp_xyz;             /* [n][3] mvpMapPoints[i]->GetWorldPos()    */
    float cam[4];                    /* fx, fy, cx, cy                           */
    float Tcw[16];                   /* mTcw, row-major 4x4 (in/out)             */
    uint8_t* outlier;                /* [n] mvbOutlier (in/out: entries with a map
                                        point are written, the rest untouched)   */
} orbx_pose_frame;

typedef struct {
    int rounds;                      /* robust rounds run (stops after round 0
                                        when the frame has < 10 edges)           */
    int iterations[4];               /* LM iterations per round                  */
    int levenberg_trials[4];         /* inner LM trials per round                */
    int n_bad[4];                    /* outliers after each round                */
    double chi2_final[4];            /* robust chi2 of the accepted state        */
    int not_posdef;                  /* LDLT failures (step rejected)            */
} orbx_pose_stats;

/* Replaces Optimizer::PoseOptimization(Frame*): updates f->Tcw and
 * f->outlier, *n_inliers = the function's return value
 * (nInitialCorrespondences - nBad).  stats may be NULL. */
int orbx_pose_optimization(orbx_ctx* ctx, orbx_pose_frame* f, int* n_inliers,
                           orbx_pose_stats* stats);
/* Batched form: P independent frames (one wavefront each, one launch). */
int orbx_pose_optimization_batch(orbx_ctx* ctx, int P, orbx_pose_frame* frames,
                                 int32_t* n_inliers, orbx_pose_stats* stats);
/* Device-resident form of the batch (bench/tests): stage P frames in HBM
 * once, run the optimisation from the staged initial poses any number of
 * times (asynchronous, on the context stream; kernel timer "pose"), fetch
 * the results of the last run into the frames' Tcw / outlier. */
int orbx_pose_stage(orbx_ctx* ctx, int P, const orbx_pose_frame* frames);
int orbx_pose_run(orbx_ctx* ctx);
int orbx_pose_fetch(orbx_ctx* ctx, orbx_pose_frame* frames, int32_t* n_inliers,
                    orbx_pose_stats* stats);
/* Summation mode of the pose optimisation (default 1).  1: every chi2 / H /
 * b sum runs sequentially in g2o's active-edge order (the edge terms are
 * computed in parallel, accumulated edge by edge), so the whole LM
 * trajectory -- accept / reject of every trial, lambda, iterations -- and
 * the returned pose are the sequential reference's bit for bit, for every
 * batch size.  0 (opt-in, faster: about 1.03x one call, 1.4x a batch): each
 * wavefront sums its edges' terms lane-strided and then through a fixed DPP
 * tree -- deterministic, but in another order than g2o, so LM steps decided
 * on rounding noise (a converged pose restarted in a later robust round) may
 * count differently: poses within 1e-5, and the result of a frame may differ
 * between a lone call (a workgroup per frame) and a batch (a wavefront per
 * frame).  Takes effect at the next orbx_pose_run.  Returns ORBX_ERR_ARG for
 * a null context or a mode outside 0..1; orbx_pose_get_exact returns the
 * mode (ORBX_ERR_ARG for NULL). */
int orbx_pose_set_exact(orbx_ctx* ctx, int exact);
int orbx_pose_get_exact(const orbx_ctx* ctx);

/* Library identification. */
const char* orbx_version(void);

#ifdef __cplusplus
}
#endif

#endif /* ORBX_H */
