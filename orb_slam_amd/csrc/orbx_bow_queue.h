// The keyframe-batch searches of orbx_bow.hip (SearchByBoW(KF1, KF2) and
// SearchForTriangulation of one keyframe against n others) as a queue step:
// validation, upload and launch without the read-back, for callers that go on
// working on the match vectors on the device (orbx_newpoints.hip).
#pragma once

#include <functional>
#include <vector>

#include "orbx_internal.h"

namespace orbx {

// What a queued batch left in the context scratch.
struct BowQueued {
    const orbx_keypoint* k1 = nullptr;       // KF1's keypoints
    uint8_t* mp1 = nullptr;                  // KF1's map-point states, read by each search launch
    std::vector<const orbx_keypoint*> k2;    // per neighbour: keypoints, their number,
    std::vector<int> n2;
    std::vector<const uint8_t*> mp2;         // its map-point states,
    std::vector<int32_t*> out, out_n;        // the match vector (out_len entries) and its count
    int n1 = 0;                              // KF1's keypoints
    int out_len = 0;
    uint8_t* extra = nullptr;                // the caller's extra_bytes (256-byte aligned)
};

// Called after neighbour k's search launch when the batch is queued serially.
using BowAfter = std::function<int(int)>;

// after == nullptr: one launch of n workgroups.  Otherwise n launches of one
// workgroup, neighbour after neighbour, (*after)(k) following each: what it
// queues on the context stream (a write to q->mp1 for instance) is seen by
// the searches of the later neighbours.  No read-back, no synchronisation
// after the launches.
int queue_bow_batch(orbx_ctx* ctx, const orbx_bow_view* V1, int n, const orbx_bow_view* V2s, int mode, float nnratio,
                    int check_ori, const float* F12s, const float* sigma2s, int nlevels, size_t extra_bytes,
                    const BowAfter* after, BowQueued* q);
int queue_bow_slots(orbx_ctx* ctx, int mode, int slot1, const uint8_t* mp1, int n, const int* slots2,
                    const uint8_t* const* mp2s, float nnratio, int check_ori, const float* F12s, const float* sigma2s,
                    int nlevels, int cap, size_t extra_bytes, const BowAfter* after, BowQueued* q);
// orbx_dev_search_by_bow (SearchByBoW(KF, F) of n keyframe views against the
// frame in `slot`) without its read-back: in *q the frame is side 1 (k1 its
// keypoints, n1 = out_len the slot capacity, mp1 unused) and keyframe k side 2
// (mp2[k] its uploaded map-point states, n2[k] its keypoints; k2 unused);
// out[k] holds the keyframe's keypoint per frame keypoint.  matches_f: the
// caller's n result arrays, checked with the other arguments.
int queue_bow_frame(orbx_ctx* ctx, int slot, int n, const orbx_bow_view* KFs, float nnratio, int check_ori,
                    int32_t* const* matches_f, int cap, size_t extra_bytes, BowQueued* q);
// The read-back of a queued batch: `len` entries of every match vector and
// the counts, as asynchronous copies on the context stream.
int read_bow_queued(orbx_ctx* ctx, const BowQueued& q, int len, int32_t* const* outs, int* n_outs);

}  // namespace orbx
