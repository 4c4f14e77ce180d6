// ORB extraction on MI355X (gfx950): ORBextractor::operator()
// (src/ORBextractor.cc:718-779) for a batch of frames, one launch per stage:
//
//   k_pyr_level0   copyMakeBorder(REFLECT_101) of the input   (:814); not
//                  launched for frames of w % 16 == 0, whose level 0 the
//                  kernels below read from the frame store (level_src)
//   k_pyr_resize_lds resize INTER_LINEAR, level l              (:800); level
//                  interiors only: no kernel of the batch path reads a
//                  border (k_describe stages the windows that leave a level
//                  from their REFLECT_101 sources inside it)
//   k_pyr_resize   the same + border (:806), per-pixel gathers: levels whose
//                  staged strip does not fit LDS
//   k_pyr_cascade  the whole raw pyramid with borders in one launch
//                  (orbx_extract's single frame)
//   k_pyr_borders  the borders of levels >= 1 of one slot (:806), on demand
//                  for orbx_dev_read_level and k_blur
//   k_fast_cells   FAST-9/16 + cell-local NMS + threshold-7
//                  fallback + raster-order compaction, one
//                  workgroup per grid cell                    (:599-614)
//   k_harris_cells HarrisResponses of every FAST corner (HARRIS_SCORE
//                  only), u64 entries keyed by the float response (:616-620)
//   k_retain_cells per-level quota redistribution + cell retainBest,
//                  one wave per cell (libstdc++ introselect)  (:622-694)
//   k_retain_levels level retainBest, one wave per level      (:697-701)
//   k_blur         GaussianBlur 7x7 sigma 2 on each level     (:760); only for
//                  orbx_dev_read_level's blurred levels
//   k_describe     IC_Angle, the GaussianBlur of the keypoint's
//                  patch, rBRIEF + coordinate scaling,
//                  two keypoints per wave                     (:124-194, :705,
//                                                              :760, :764-777)
//
// All integer / byte work; the bounds are HBM or latency, never MFMA.
#include <algorithm>
#include <type_traits>

#include "orbx_device.h"
#include "orbx_internal.h"

namespace orbx {

constexpr size_t kRetainLds = 128 * 1024;   // LDS budget of a retain block
constexpr int kRetainCellCap = 512;         // cell lists up to this length sort in LDS
constexpr int kSplitMinFrames = 16;         // batches >= 2x this run as two concurrent halves
constexpr size_t kResizeLds = 96 * 1024;    // LDS budget of a staged resize strip

__constant__ __attribute__((aligned(4))) int8_t c_pattern[256][4] = {
#include "orbx_pattern.inc"
};

#ifdef ORBX_FAST_PROFILE
__device__ unsigned long long g_fast_prof[32];
__device__ inline unsigned long long fp_stamp()
{
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}
#define FP_T0() unsigned long long _ft = fp_stamp()
#define FP_MARK(k)                                                                  \
    do {                                                                            \
        const unsigned long long _n = fp_stamp();                                   \
        if (threadIdx.x == 0) atomicAdd(&g_fast_prof[k], _n - _ft);                 \
        _ft = _n;                                                                   \
    } while (0)
#define FP_ADD(k, v) atomicAdd(&g_fast_prof[k], (unsigned long long)(v))
extern "C" int orbx_debug_fast_prof(unsigned long long* out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fast_prof), sizeof(unsigned long long) * 32) == hipSuccess ? 0 : -2;
}
#else
#define FP_T0()
#define FP_MARK(k)
#define FP_ADD(k, v)
#endif

struct ExtractArgs {
    const LevelGeom* levels;
    const CellGeom* cells;
    const ResizeCol* res_cols;
    const ResizeRow* res_rows;
    const uint32_t* ic_rows;   // ic_row_table: IC_Angle's circle, by rows
    const uint8_t* frames;
    uint8_t* pyr_raw;
    uint8_t* pyr_blur;
    uint32_t* cell_lists;
    int32_t* cell_count;
    uint8_t* fast_path;             // slots x ncells (all slots, indexed from first_slot): k_fast_cells' path per cell
    uint32_t* level_keys;
    int32_t* level_count;
    orbx_keypoint* out_kps;
    uint8_t* out_desc;
    int32_t* out_n;
    int32_t* error_flags;
    // orbx_extract's single frame: k_describe also writes the page-locked
    // read-back block (count and flags at 0, records at 64, descriptors
    // after nfeatures records), in place of a pack launch; else null
    uint8_t* host_out;
    int32_t* retain_scratch;        // slots x (list_entries + 4 ncells): global nth_element scratch
    uint64_t* cell_keys64;          // HARRIS_SCORE: Harris-keyed cell lists (as cell_lists)
    uint64_t* level_keys64;         // HARRIS_SCORE: Harris-keyed level lists (as level_keys)
    int harris;                     // scoreType == HARRIS_SCORE
    int fp_contract;                // orbx_set_fp_contract: FMA-contracted reference build
    int nth_pivot;                  // orbx_set_nth_pivot: retainBest's libstdc++ era
    long long frame_pyr_bytes;
    int first_slot;
    int w, h;
    int nlevels, ncells, list_entries, level_entries, nfeatures;
    int fast_th, fast_th_low;       // FAST thresholds (fastTh, 7), clamped
    int max_list_cap, max_level_cap;
    // level 0 is read from the frame store (no k_pyr_level0 copy): frame width
    // a multiple of 16, not the single-frame cascade (launch_extract)
    int l0_direct;
};

// A level's padded origin and row stride for frame f of the pass (off and
// stride: the level's LevelGeom entries).  Level 0 in direct mode is the
// frame itself: its virtual padded origin, kEdge rows and columns in front of
// the frame's first pixel, with row stride w.  Only addresses inside the
// image may be read through it -- the border does not exist there.  With
// kEdge == 16 and w % 16 == 0 the origin keeps the 16-byte alignment of the
// padded level, and interior addressing (kEdge + y) * stride + kEdge + x is
// unchanged.
struct LevelSrc {
    const uint8_t* base;
    int stride;
};
static_assert(kEdge % 16 == 0, "the direct level 0 keeps the padded level's 16-byte alignment");
__device__ __forceinline__ LevelSrc level_src(const ExtractArgs& a, int f, int level, long long off, int stride)
{
    if (a.l0_direct && level == 0)
        return {a.frames + ((long long)(a.first_slot + f) * a.w * a.h - (long long)kEdge * a.w - kEdge), a.w};
    return {a.pyr_raw + (size_t)f * a.frame_pyr_bytes + off, stride};
}

// The geometry tables (cells, levels, ...) are never written by a kernel:
// read through the constant address space, a wave-uniform read is a scalar
// load (scalar cache hit once warm) instead of a vector load + readfirstlane,
// so the dependent table reads in front of a workgroup's first data loads
// cost cache hits rather than L2 round trips.
template <class T>
__device__ __forceinline__ T cget(const T* p, int i)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return ((const __attribute__((address_space(4))) T*)p)[i];
#else
    return p[i];   // host pass: parsed, never called
#endif
}

__device__ inline uint8_t sat_u8(int v) { return (uint8_t)min(max(v, 0), 255); }
__device__ inline int sat_s16(int v) { return min(max(v, -32768), 32767); }

// Copy n items into LDS, kBatch per thread per round: the loads are
// unconditional (index clamped to n - 1, whose entry out-of-range lanes
// rewrite with its own value), so no branch separates them and all kBatch
// are in flight before the first wait.
template <int kBatch, typename T, typename Load>
__device__ inline void stage_to_lds(T* dst, int n, int tid, int nthr, Load load)
{
    for (int u0 = 0; u0 < n; u0 += kBatch * nthr) {
        T v[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) v[k] = load(min(u0 + k * nthr + tid, n - 1));
#pragma unroll
        for (int k = 0; k < kBatch; k++) dst[min(u0 + k * nthr + tid, n - 1)] = v[k];
    }
}

// ---------------------------------------------------------------------------
// Level 0: padded copy with BORDER_REFLECT_101.  16 output bytes per thread
// and row: interior words are two aligned 16-byte loads funnel-shifted by
// the border offset; words touching the border gather reflected bytes.
// ---------------------------------------------------------------------------
// One thread per (16-byte column, strip of kPyrRows rows): the strip's
// independent row loads are in flight together.
constexpr int kPyrRows = 8;
constexpr int kPyr0Shift = (16 - kEdge % 16) % 16;   // (16q - kEdge) mod 16

// Work items: first the interior words (q_lo .. q_lo + nint - 1) in strips of
// kPyrRows rows, then the border words one (word, row) each, so border
// gathers run in waves of their own.
__global__ __launch_bounds__(256) void k_pyr_level0(ExtractArgs a, int q_lo, int nint)
{
    const int f = blockIdx.y;
    const LevelGeom L = cget(a.levels, 0);
    const int qpr = L.stride >> 4, nstrips = (L.ph + kPyrRows - 1) / kPyrRows;
    const int nbord = qpr - nint;
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const uint8_t* src = a.frames + (size_t)(a.first_slot + f) * a.w * a.h;
    uint8_t* dst = a.pyr_raw + (size_t)f * a.frame_pyr_bytes + L.off;
    if (idx < nint * nstrips) {
        const int strip = idx / nint, q = q_lo + (idx - strip * nint), px0 = 16 * q;
        const int al = px0 - kEdge - kPyr0Shift;   // 16-byte aligned source column
        const int py_first = strip * kPyrRows;
        // all the strip's loads first (rows past the level repeat the last
        // one, their stores are skipped), then the funnel shifts and stores
        uint4 lo[kPyrRows], hi[kPyrRows];
#pragma unroll
        for (int rr = 0; rr < kPyrRows; rr++) {
            const int py = min(py_first + rr, L.ph - 1);
            const uint8_t* row = src + (size_t)reflect101(py - kEdge, L.h) * a.w + al;
            lo[rr] = *reinterpret_cast<const uint4*>(row);
            hi[rr] = *reinterpret_cast<const uint4*>(row + 16);
        }
#pragma unroll
        for (int rr = 0; rr < kPyrRows; rr++) {
            const uint32_t w[8] = {lo[rr].x, lo[rr].y, lo[rr].z, lo[rr].w, hi[rr].x, hi[rr].y, hi[rr].z, hi[rr].w};
            constexpr int d = kPyr0Shift >> 2, b = kPyr0Shift & 3;
            uint32_t o[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                o[k] = b ? __builtin_amdgcn_alignbyte(w[k + d + 1], w[k + d], b) : w[k + d];
            if (py_first + rr < L.ph)
                *reinterpret_cast<uint4*>(dst + (size_t)(py_first + rr) * L.stride + px0) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        return;
    }
    idx -= nint * nstrips;
    if (idx >= nbord * L.ph) return;
    const int py = idx / nbord, k = idx - py * nbord;
    const int q = k < q_lo ? k : k + nint, px0 = 16 * q;
    const uint8_t* row = src + (size_t)reflect101(py - kEdge, L.h) * a.w;
    if (kEdge == 16 && a.w % 16 == 0 && a.w >= 32) {
        // aligned rows: the left border word is frame bytes 16 .. 1, the word
        // after the last 16 interior bytes is bytes w-2 .. w-17 (byte permutes
        // of two aligned loads), the rest of the row is zero
        const int w16 = a.w >> 4;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (q == 0) {
            const uint4 A = *reinterpret_cast<const uint4*>(row), B = *reinterpret_cast<const uint4*>(row + 16);
            v.x = __builtin_amdgcn_perm(B.x, A.w, 0x01020304u);
            v.y = __builtin_amdgcn_perm(A.w, A.z, 0x01020304u);
            v.z = __builtin_amdgcn_perm(A.z, A.y, 0x01020304u);
            v.w = __builtin_amdgcn_perm(A.y, A.x, 0x01020304u);
        } else if (q <= w16) {
            v = *reinterpret_cast<const uint4*>(row + 16 * (q - 1));
        } else if (q == w16 + 1) {
            const uint4 A = *reinterpret_cast<const uint4*>(row + a.w - 32), B = *reinterpret_cast<const uint4*>(row + a.w - 16);
            v.x = __builtin_amdgcn_perm(B.w, B.z, 0x03040506u);
            v.y = __builtin_amdgcn_perm(B.z, B.y, 0x03040506u);
            v.z = __builtin_amdgcn_perm(B.y, B.x, 0x03040506u);
            v.w = __builtin_amdgcn_perm(B.x, A.w, 0x03040506u);
        }
        *reinterpret_cast<uint4*>(dst + (size_t)py * L.stride + px0) = v;
        return;
    }
    uint8_t v[16];
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = px0 + i < L.pw ? row[reflect101(px0 + i - kEdge, L.w)] : 0;
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
        o[i] = v[4 * i] | (uint32_t)v[4 * i + 1] << 8 | (uint32_t)v[4 * i + 2] << 16 | (uint32_t)v[4 * i + 3] << 24;
    *reinterpret_cast<uint4*>(dst + (size_t)py * L.stride + px0) = make_uint4(o[0], o[1], o[2], o[3]);
}

// ---------------------------------------------------------------------------
// Level l >= 1: cv::resize INTER_LINEAR from level l-1 (fixed point, 11-bit
// weights; columns < nvec use the SSE2 VResizeLinearVec_32s8u arithmetic,
// the rest the scalar FixedPtCast<int,uchar,22>), then copyMakeBorder
// REFLECT_101 of the level itself (border pixels recompute their source).
// ---------------------------------------------------------------------------
__device__ inline uint8_t resize_pixel(const uint8_t* prev, int pstride, const ResizeCol& c,
                                       const ResizeRow& r, bool vec)
{
    const uint8_t* r0 = prev + (size_t)r.sy0 * pstride;
    const uint8_t* r1 = prev + (size_t)r.sy1 * pstride;
    const int S0 = r0[c.sx0] * c.a0 + r0[c.sx1] * c.a1;
    const int S1 = r1[c.sx0] * c.a0 + r1[c.sx1] * c.a1;
    if (vec) {
        const int x0 = sat_s16(S0 >> 4), y0 = sat_s16(S1 >> 4);
        int v = sat_s16(((x0 * r.b0) >> 16) + ((y0 * r.b1) >> 16));
        v = sat_s16(v + 2) >> 2;
        return sat_u8(v);
    }
    return sat_u8((S0 * r.b0 + S1 * r.b1 + (1 << 21)) >> 22);
}

__global__ __launch_bounds__(256) void k_pyr_resize(ExtractArgs a, int level)
{
    const int f = blockIdx.y;
    const LevelGeom L = cget(a.levels, level);
    const LevelGeom P = cget(a.levels, level - 1);
    const int wpr = L.stride >> 2, nstrips = (L.ph + kPyrRows - 1) / kPyrRows;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= wpr * nstrips) return;
    const int strip = idx / wpr, q = idx - strip * wpr, px0 = 4 * q;
    // interior sources only (the level's own border recomputes its source)
    const LevelSrc ps = level_src(a, f, level - 1, P.off, P.stride);
    const uint8_t* prev = ps.base + (size_t)kEdge * ps.stride + kEdge;
    uint8_t* dst = a.pyr_raw + (size_t)f * a.frame_pyr_bytes + L.off;
    ResizeCol c[4];
    bool vec[4], on[4];
#pragma unroll
    for (int b = 0; b < 4; b++) {
        on[b] = px0 + b < L.pw;
        const int x = on[b] ? reflect101(px0 + b - kEdge, L.w) : 0;
        c[b] = a.res_cols[L.res_col_off + x];
        vec[b] = x < L.nvec_resize;
    }
#pragma unroll
    for (int rr = 0; rr < kPyrRows; rr++) {
        const int py = min(strip * kPyrRows + rr, L.ph - 1);
        const ResizeRow r = a.res_rows[L.res_row_off + reflect101(py - kEdge, L.h)];
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (on[b]) word |= (uint32_t)resize_pixel(prev, ps.stride, c[b], r, vec[b]) << (8 * b);
        if (strip * kPyrRows + rr < L.ph) *reinterpret_cast<uint32_t*>(dst + (size_t)py * L.stride + px0) = word;
    }
}

// The same resize with the strip's source rows staged in LDS, for the
// level's interior only: one workgroup per (strip of kResRows interior rows,
// frame), rows 1:1 with the row table.  Nothing on the batch path reads a
// level's border (the next level's resize stages interior sources, FAST and
// Harris cells lie inside the level, k_describe reflects the windows that
// leave it), so no border row, border word or row padding is computed or
// stored here: launch_borders_slot fills them for the readers of a padded
// level.  The previous level's interior rows [lo, hi] feeding the strip are
// copied with 16-byte loads from their first interior byte (columns
// 0 .. P.w - 1 and up to 15 bytes behind them), together with the level's
// column and row tables; every output pixel then reads its 2x2 sources from
// LDS.  The bytes behind column P.w - 1 belong to the parent's border or
// padding (allocated, maybe never written; the frame's next row for the
// direct level 0, whose width is a multiple of 16, so none is staged there).
// Only the second tap of the HResizeLinear tail columns reads one of them
// (sx0 = P.w - 1, tap at +1), with weight a1 = 0: the value never reaches a
// result.  Every other tap has sx0 + 1 <= P.w - 1 (resize_tables).
// The host guarantees hi - lo + 1 <= L.res_span (computed from the tables).
// The level's and its parent's geometry, passed by value: no dependent
// table read before the staging loads.
struct ResizeLevel {
    long long off, poff;                 // level / parent offsets in a frame's pyramid
    int stride, pstride, w, h, ph_parent_h, nvec, span, strip_off, row_off, col_off;
    int packed;                          // every interior word's taps lie within 8 bytes (the packed form applies)
    int plevel;                          // the parent's level index (level_src: level 0 may be the frame itself)
    // Interior words [0, nslide) run the sliding form in whole waves; the
    // other rem = nfast - nslide < 64 go to wave rem_wave as (row group,
    // word) items, rem_n rows per group (0: no remainder).  The host leaves
    // nslide = nfast where fewer than two groups fit a wave.
    int nslide, rem_wave, rem_n;
};

__global__ __launch_bounds__(256) void k_pyr_resize_lds(ExtractArgs a, ResizeLevel L, int pitch)
{
    extern __shared__ uint4 s_dyn[];
    __shared__ ResizeRow s_rows[kResRows];
    __shared__ __attribute__((aligned(16))) uint2 s_slide[kResRows];
    const int f = blockIdx.y, tid = threadIdx.x;
    const int y0 = blockIdx.x * kResRows, nrows = min(kResRows, L.h - y0);   // interior rows y0 .. y0 + nrows - 1
    const int nch = pitch >> 4;
    ResizeCol* s_cols = reinterpret_cast<ResizeCol*>(s_dyn + (size_t)L.span * nch);
    uint8_t* s_src = reinterpret_cast<uint8_t*>(s_dyn);
    // the strip's first source row comes from a host table (uniform scalar
    // load), so the staging loads go out together with the row/column tables
    const int lo = a.res_rows[L.strip_off + blockIdx.x].sy0;
    if (tid < nrows) {
        const ResizeRow e = a.res_rows[L.row_off + y0 + tid];
        s_rows[tid] = e;
        // The sliding form's copy of the entry carries in the free bit 12 of
        // b0 (weights are <= 2048) whether the row's first source row is new:
        // not the previous row's second, which the sliding form still holds.
        // Decided here once per strip, not per wave and row.
        const ResizeRow p = a.res_rows[L.row_off + y0 + max(tid, 1) - 1];
        const uint32_t first = (tid == 0 || p.sy1 != e.sy0) ? 0x1000u : 0u;
        s_slide[tid] = make_uint2((uint32_t)(uint16_t)e.sy0 | (uint32_t)(uint16_t)e.sy1 << 16,
                                  (uint32_t)(uint16_t)e.b0 | first | (uint32_t)(uint16_t)e.b1 << 16);
    }
    stage_to_lds<4>(s_cols, L.w, tid, (int)blockDim.x, [&](int x) { return a.res_cols[L.col_off + x]; });
    const int nsrc = min(L.span, L.ph_parent_h - lo);
    // parent row lo from its first interior byte (16-byte aligned in the
    // padded level and in the frame); rows lo .. lo + nsrc - 1 < P.h.  For the
    // frame every staged byte lies inside it (pitch = P.w)
    const LevelSrc ps = level_src(a, f, L.plevel, L.poff, L.pstride);
    const uint8_t* pbase = ps.base + (size_t)(lo + kEdge) * ps.stride + kEdge;
#ifndef RES_NO_STAGE
    {
        // u / nch as a float product: (u + 1/2) / nch lies at least 1/(2 nch)
        // from an integer and the product errs by < 2^-21 (u + 1) for
        // u < 2^16 (no integer division per item)
        const float inv = 1.0f / (float)nch;
        stage_to_lds<8>(s_dyn, nsrc * nch, tid, (int)blockDim.x, [&](int u) {
            const int r = (int)(((float)u + 0.5f) * inv), c = u - r * nch;
            return *reinterpret_cast<const uint4*>(pbase + (size_t)r * ps.stride + 16 * c);
        });
    }
#endif
    __syncthreads();
    uint8_t* dst = a.pyr_raw + (size_t)f * a.frame_pyr_bytes + L.off + (size_t)(kEdge + y0) * L.stride;
#ifdef RES_NO_COMPUTE
    if (tid < 64) reinterpret_cast<uint32_t*>(dst)[tid] = s_src[tid * 7];
    return;
#endif
    // Output words split by form (one after the other: no wave runs two forms
    // under a per-lane branch):
    //  * interior words [q_lo, q_hi) whose four columns are on the SSE2 path
    //    (x < nvec): the packed form below, one thread per word sliding
    //    down the strip's rows in whole waves, the last nfast % 64 words as
    //    (row group, word) items of one wave (ResizeLevel::nslide);
    //  * the other words holding an interior column (a scalar-tail column
    //    x >= nvec, a word straddling nvec or w; every interior word of a
    //    level that is not packed): one (row, word) item per thread, in the
    //    general form.
    // sx1 is sx0 + 1, or sx0 with a1 = 0 (HResizeLinear tail), so the
    // second tap is always read at offset +1.
    const int q_lo = (kEdge + 3) >> 2, q_hi = L.packed ? max(q_lo, (kEdge + min(L.w, L.nvec)) >> 2) : q_lo;
    const int nfast = q_hi - q_lo;
    // Packed form: a word's four source taps lie in 8 bytes (source step
    // < 2, so sx0(x + 3) - sx0(x) <= 6); three dword reads aligned to the
    // word's first tap (alignbyte) hold them, each column's (p0, p1) pair is
    // one v_perm into 16-bit halves and its 2-tap sum one v_dot2_u32_u16 with
    // weights (16 a0, 16 a1) -- 16 S, whose bits 8..23 are (S >> 4) << 8 --
    // and VResizeLinearVec_32s8u's (S >> 4) * b >> 16 is one
    // v_mul_hi_u32_u24 of that with b << 8.  S >> 4 <= 32640 and the
    // weights are <= 2048, so none of its 16-bit saturations can trigger;
    // the rounded row weights sum to 2048 +- 1 (cvRound of complementary
    // values), so the two terms sum to <= 32640 * 2049 / 2^16 < 1021, the
    // final (t + 2) >> 2 is <= 255 and its u8 saturation is a no-op.
    typedef unsigned short orbx_us2 __attribute__((ext_vector_type(2)));
    auto mh = [](uint32_t x, uint32_t y) {   // bits 32..47 of the 24 x 24-bit product
        return (uint32_t)(((unsigned long long)(x & 0xFFFFFFu) * (unsigned long long)(y & 0xFFFFFFu)) >> 32);
    };
    // Word q_lo + t over the strip's rows [r0, r1).  kUni: the whole wave
    // walks the same rows (the sliding form), so which source rows a row
    // needs is wave-uniform.
    auto word_rows = [&](auto uni, int t, int r0, int r1) {
        constexpr bool kUni = decltype(uni)::value;
        const int q = q_lo + t, x0 = 4 * q - kEdge;
        int ca[4];
        uint32_t sel[4], wgt[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const ResizeCol c = s_cols[x0 + b];
            ca[b] = c.sx0;
            wgt[b] = (uint32_t)(16 * c.a0) | (uint32_t)(16 * c.a1) << 16;
        }
        const int qa = ca[0] & ~3, sh = ca[0] & 3;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t r = (uint32_t)(ca[b] - ca[0]);   // tap bytes r, r + 1 of the aligned 8 (L.packed)
            sel[b] = r | 0x0C00u | (r + 1) << 16 | 0x0C000000u;
        }
        auto hrow = [&](int sy, uint32_t (&S)[4]) {
            const uint32_t* d = reinterpret_cast<const uint32_t*>(s_src + (sy - lo) * pitch + qa);
            const uint32_t d0 = d[0], d1 = d[1], d2 = d[2];
            const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, sh), w1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
#pragma unroll
            for (int b = 0; b < 4; b++)
                S[b] = __builtin_amdgcn_udot2(__builtin_bit_cast(orbx_us2, __builtin_amdgcn_perm(w1, w0, sel[b])),
                                              __builtin_bit_cast(orbx_us2, wgt[b]), 0u, false) &
                       0x00FFFF00u;
        };
        uint8_t* out = dst + (size_t)r0 * L.stride + 4 * q;
        if constexpr (kUni) {
            // The whole strip (r0 == 0: s_slide's flags count from its first
            // row).  Two register sets hold the horizontal sums of a row's
            // two source rows.  A row computes its second source row over
            // the set that held the previous row's first, and its first only
            // if that is not the previous row's second (s_slide's flag); then
            // the sets swap roles.  The loop takes two rows per trip, one per
            // role assignment: no sums are copied from set to set, and no
            // wave compares source rows.
            static_assert(kResRows % 2 == 0, "the sliding form reads s_slide in pairs");
            uint32_t X[4], Y[4];
            auto row = [&](const uint32_t w0, const uint32_t w1, uint32_t (&P)[4], uint32_t (&Q)[4]) {
                const uint32_t B0 = (w1 & 0xFFFu) << 8, B1 = (w1 >> 16) << 8;
                if (w1 & 0x1000u) {
                    asm volatile("; first source row");   // (a branch, not a select over both sets)
                    hrow((int)(w0 & 0xFFFFu), Q);
                }
                hrow((int)(w0 >> 16), P);
                uint32_t word = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) word |= ((mh(Q[b], B0) + mh(P[b], B1) + 2) >> 2) << (8 * b);
                *reinterpret_cast<uint32_t*>(out) = word;
                out += L.stride;
            };
            // a pair's entries go to scalar registers before the next pair's
            // are read over them, a trip ahead of their use (the last trip
            // reads the last pair again, not past the table)
            int rr = 0;
            uint4 e = *reinterpret_cast<const uint4*>(s_slide);
            for (; rr + 1 < r1; rr += 2) {
                const uint32_t a0 = __builtin_amdgcn_readfirstlane(e.x), a1 = __builtin_amdgcn_readfirstlane(e.y);
                const uint32_t c0 = __builtin_amdgcn_readfirstlane(e.z), c1 = __builtin_amdgcn_readfirstlane(e.w);
                e = *reinterpret_cast<const uint4*>(s_slide + min(rr + 2, kResRows - 2));
                row(a0, a1, X, Y);
                row(c0, c1, Y, X);
            }
            if (rr < r1) row(__builtin_amdgcn_readfirstlane(e.x), __builtin_amdgcn_readfirstlane(e.y), X, Y);
            return;
        }
        // A row group of the remainder wave: rows differ from lane to lane,
        // so the entries and the reuse of the previous row's sums (H0, H1:
        // source rows c0, c1) are per lane.  The next row's table entry is
        // read while this row is computed.
        uint2 nxt = reinterpret_cast<const uint2*>(s_rows)[r0];
        uint32_t H0[4], H1[4];
        int c0 = -1, c1 = -1;
        for (int rr = r0; rr < r1; rr++, out += L.stride) {
            const uint2 cur = nxt;
            if (rr + 1 < r1) nxt = reinterpret_cast<const uint2*>(s_rows)[rr + 1];
            const uint32_t w0 = cur.x, w1 = cur.y;
            const int sy0 = (int)(int16_t)(w0 & 0xFFFF), sy1 = (int)(int16_t)(w0 >> 16);
            const uint32_t B0 = (w1 & 0xFFFFu) << 8, B1 = (w1 >> 16) << 8;
            uint32_t A[4], B[4];
            if (sy0 == c1) {
#pragma unroll
                for (int b = 0; b < 4; b++) A[b] = H1[b];
            } else if (sy0 == c0) {
#pragma unroll
                for (int b = 0; b < 4; b++) A[b] = H0[b];
            } else {
                hrow(sy0, A);
            }
            if (sy1 == sy0) {
#pragma unroll
                for (int b = 0; b < 4; b++) B[b] = A[b];
            } else if (sy1 == c1) {
#pragma unroll
                for (int b = 0; b < 4; b++) B[b] = H1[b];
            } else {
                hrow(sy1, B);
            }
#pragma unroll
            for (int b = 0; b < 4; b++) {
                H0[b] = A[b];
                H1[b] = B[b];
            }
            c0 = sy0;
            c1 = sy1;
            uint32_t word = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) word |= ((mh(A[b], B0) + mh(B[b], B1) + 2) >> 2) << (8 * b);
            *reinterpret_cast<uint32_t*>(out) = word;
        }
    };
    const int rem = nfast - L.nslide;
    for (int t = tid; t < L.nslide; t += blockDim.x) word_rows(std::true_type{}, t, 0, nrows);
    if (rem > 0 && __builtin_amdgcn_readfirstlane(tid >> 6) == L.rem_wave) {
        // lane -> (row group g, word lane - g rem); lane / rem as a float
        // product (lane < 64: exact)
        const int lane = tid & 63, g = (int)(((float)lane + 0.5f) * (1.0f / (float)rem));
        // rem_n = ceil(kResRows / (64 / rem)): the groups tile the strip, and
        // the lanes past the last whole group start at or after its end
        const int r0 = g * L.rem_n;
        if (r0 < nrows) word_rows(std::false_type{}, L.nslide + lane - g * rem, r0, min(r0 + L.rem_n, nrows));
    }
    // The general form of one output word: per byte the column (reflected
    // for the up to three border bytes behind the last interior column, which
    // thus hold copyMakeBorder's values), its two taps in both source rows and
    // the column's rounding (SSE2 path or FixedPtCast<int, uchar, 22>).
    auto general_word = [&](int rr, int q) {
        const int px0 = 4 * q;
        const ResizeRow R = s_rows[rr];
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int x = reflect101(px0 + b - kEdge, L.w);
            const ResizeCol c = s_cols[x];
            const uint8_t* r0 = s_src + (R.sy0 - lo) * pitch + c.sx0;
            const uint8_t* r1 = s_src + (R.sy1 - lo) * pitch + c.sx0;
            const int S0 = r0[0] * c.a0 + r0[1] * c.a1, S1 = r1[0] * c.a0 + r1[1] * c.a1;
            int v;
            if (x < L.nvec)
                v = (((S0 >> 4) * R.b0 >> 16) + ((S1 >> 4) * R.b1 >> 16) + 2) >> 2;
            else   // FixedPtCast<int, uchar, 22>
                v = (S0 * R.b0 + S1 * R.b1 + (1 << 21)) >> 22;
            word |= (uint32_t)sat_u8(v) << (8 * b);
        }
        *reinterpret_cast<uint32_t*>(dst + (size_t)rr * L.stride + px0) = word;
    };
    // the words [q_hi, q_in) by the workgroup's last threads (the waves with
    // the least packed work)
    const int q_in = (kEdge + L.w + 3) >> 2, ntail = q_in - q_hi;
    for (int item = (int)blockDim.x - 1 - tid; item < kResRows * ntail; item += blockDim.x) {
        const int rr = item % kResRows;
        if (rr < nrows) general_word(rr, q_hi + item / kResRows);
    }
}

// ---------------------------------------------------------------------------
// The whole raw pyramid in one launch: ComputePyramid (src/ORBextractor.cc:
// 781-822) as a cascade of row bands.  One workgroup per (band, frame) walks
// the levels: level 0's rows come from the frame, level l's from level
// l - 1's rows in LDS (ping-pong buffers, each row in the padded layout), so
// no level waits for another launch.  Per (band, level) the host plan gives
// the padded rows the band writes (a partition of the level) and the ROI
// rows it computes: those rows' sources plus every ROI row the band's share
// of the next level reads (a few halo rows are computed by two bands, with
// the same arithmetic).  Each ROI pixel is the staged resize's (the row /
// column tables, the SSE2 column path and the scalar tail), the border
// pixels copyMakeBorder's REFLECT_101 copies of it, bytes past the padded
// width zero: the buffers equal the staged launches', byte for byte.
// plan[band * nlevels + l] = (first owned ROI row, end, first computed ROI
// row, last computed ROI row); a band writes its owned rows' padded rows and
// the border rows that reflect to them.
// ---------------------------------------------------------------------------
// T threads per workgroup: 256 in batches (several bands per CU), 1024 for
// orbx_extract's single frame, whose ~23 bands leave most CUs idle: more
// threads per band shorten each level's row loop.
#ifndef ORBX_CASCADE_SINGLE_THREADS
#define ORBX_CASCADE_SINGLE_THREADS 1024
#endif
#ifdef ORBX_CASC_PROFILE
// diagnostic: band 0's cycles per (level, phase): 0 resize or level-0 load,
// 1 first barrier, 2 border pass + second barrier, 3 pyramid stores
__device__ unsigned long long g_casc_prof[kMaxLevels][4];
#define CASC_T0() unsigned long long _ct = __builtin_readcyclecounter()
#define CASC_MARK(l, k)                                                          \
    do {                                                                         \
        const unsigned long long _n = __builtin_readcyclecounter();              \
        if (blockIdx.x == 0 && threadIdx.x == 0) g_casc_prof[l][k] += _n - _ct;  \
        _ct = _n;                                                                \
    } while (0)
extern "C" int orbx_debug_casc_prof(unsigned long long* out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_casc_prof), sizeof(g_casc_prof)) == hipSuccess ? 0 : -2;
}
#else
#define CASC_T0()
#define CASC_MARK(l, k)
#endif
// kTab (the single-frame instance): every level's column table and the
// band's row-table slices are staged in LDS at tab_off (tab_cols entries,
// then the rows) with the level-0 loads, so no level's row loop waits on a
// global table load per row (band 0's stamps: 4-5 dependent ~2 k-cycle
// loads per group at levels 1-3 before).
template <int T>
__global__ __launch_bounds__(T) void k_pyr_cascade(ExtractArgs a, const int4* plan, int buf_x, int tab_off,
                                                   int tab_cols)
{
    CASC_T0();
    const bool kTab = T >= 1024 && tab_off > 0;   // tab_off 0: tables too large for LDS, read from HBM
    extern __shared__ uint4 s_dyn[];
    uint8_t* const lds = reinterpret_cast<uint8_t*>(s_dyn);   // buffers: [0, buf_x) even levels, then odd
    const int band = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    uint8_t* pyr = a.pyr_raw + (size_t)f * a.frame_pyr_bytes;
    const uint8_t* img = a.frames + (size_t)(a.first_slot + f) * a.w * a.h;
    ResizeCol* const t_cols = reinterpret_cast<ResizeCol*>(lds + tab_off);
    ResizeRow* const t_rows = reinterpret_cast<ResizeRow*>(t_cols + tab_cols);
    if (kTab) {
        // flat index over the levels' column tables, then the band's row
        // slices; four loads in flight per thread before the stores
        int ncol = 0, nrow = 0;
        for (int l = 1; l < a.nlevels; l++) {
            const int4 pl = plan[band * a.nlevels + l];
            ncol += cget(a.levels, l).w;
            nrow += max(0, pl.w - pl.z + 1);
        }
        const int n = ncol + nrow;
        for (int u0 = 0; u0 < n; u0 += 4 * T) {
            uint2 v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                int e = u0 + k * T + tid;
                v[k] = make_uint2(0, 0);
                if (e >= n) continue;
                if (e < ncol) {
                    int l = 1, w;
                    while (e >= (w = cget(a.levels, l).w)) {
                        e -= w;
                        l++;
                    }
                    v[k] = *reinterpret_cast<const uint2*>(a.res_cols + cget(a.levels, l).res_col_off + e);
                } else {
                    e -= ncol;
                    int l = 1, m;
                    int4 pl = plan[band * a.nlevels + 1];
                    while (e >= (m = max(0, pl.w - pl.z + 1))) {
                        e -= m;
                        l++;
                        pl = plan[band * a.nlevels + l];
                    }
                    v[k] = *reinterpret_cast<const uint2*>(a.res_rows + cget(a.levels, l).res_row_off + pl.z + e);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int e = u0 + k * T + tid;
                if (e < ncol) reinterpret_cast<uint2*>(t_cols)[e] = v[k];
                else if (e < n) reinterpret_cast<uint2*>(t_rows)[e - ncol] = v[k];
            }
        }
    }
    int sc0 = 0, sstride = 0;   // the previous level's first computed ROI row and row pitch
    int tcol = 0, trow = 0;     // this level's offsets in the staged tables (kTab)
    for (int l = 0; l < a.nlevels; l++) {
        const int4 pl = plan[band * a.nlevels + l];
        const LevelGeom L = cget(a.levels, l);
        const int stride = L.stride, c0 = pl.z, nrows = pl.w - pl.z + 1;
        uint8_t* dst = lds + (l & 1) * buf_x;
        // 1. the ROI rows [c0, c0 + nrows) into dst at byte kEdge of each row
        if (l == 0) {
            // the frame's rows, 16-byte loads (w % 16 == 0: host), four in
            // flight per thread before the first store
            const int n16 = a.w >> 4, n = nrows * n16;
            for (int u0 = 0; u0 < n; u0 += 4 * T) {
                uint4 v[4];
                int o[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int u = min(u0 + k * T + tid, n - 1), r = u / n16, q = u - r * n16;
                    v[k] = *reinterpret_cast<const uint4*>(img + (size_t)(c0 + r) * a.w + 16 * q);
                    o[k] = r * stride + kEdge + 16 * q;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) *reinterpret_cast<uint4*>(dst + o[k]) = v[k];
            }
        } else if (nrows > 0) {
            const uint8_t* src = lds + ((l - 1) & 1) * buf_x;
            // one thread per 4-pixel word and group of rows (G groups when the
            // row is at most T / G words wide; wider rows loop over words)
            const int nw = (L.w + 3) >> 2;
            const int G = max(1, T / nw), g = tid / nw;
            for (int q = tid - min(g, G - 1) * nw; g < G && q < nw; q += T) {
                const int r_lo = g * nrows / G, r_hi = (g + 1) * nrows / G;
                const int px0 = 4 * q;
                int ca[4], a0[4], a1[4];
                bool vb[4], vec = true;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const bool on = px0 + b < L.w;
                    const ResizeCol c = kTab ? t_cols[tcol + (on ? px0 + b : 0)] : a.res_cols[L.res_col_off + (on ? px0 + b : 0)];
                    ca[b] = kEdge + c.sx0;
                    a0[b] = on ? c.a0 : 0;
                    a1[b] = on ? c.a1 : 0;
                    vb[b] = px0 + b < L.nvec_resize;
                    vec = vec && (!on || vb[b]);
                }
                auto hrow = [&](int sy, int (&S)[4]) {
                    const uint8_t* base = src + (sy - sc0) * sstride;
#pragma unroll
                    for (int b = 0; b < 4; b++) S[b] = base[ca[b]] * a0[b] + base[ca[b] + 1] * a1[b];
                };
                int H0[4], H1[4], cs0 = -1, cs1 = -1;
                for (int r = r_lo; r < r_hi; r++) {
                    const ResizeRow rw = kTab ? t_rows[trow + r] : a.res_rows[L.res_row_off + c0 + r];
                    const int sy0 = rw.sy0, sy1 = rw.sy1, b0 = rw.b0, b1 = rw.b1;
                    int A[4], B[4];
                    if (sy0 == cs1) {
#pragma unroll
                        for (int b = 0; b < 4; b++) A[b] = H1[b];
                    } else if (sy0 == cs0) {
#pragma unroll
                        for (int b = 0; b < 4; b++) A[b] = H0[b];
                    } else {
                        hrow(sy0, A);
                    }
                    if (sy1 == sy0) {
#pragma unroll
                        for (int b = 0; b < 4; b++) B[b] = A[b];
                    } else if (sy1 == cs1) {
#pragma unroll
                        for (int b = 0; b < 4; b++) B[b] = H1[b];
                    } else {
                        hrow(sy1, B);
                    }
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        H0[b] = A[b];
                        H1[b] = B[b];
                    }
                    cs0 = sy0;
                    cs1 = sy1;
                    uint32_t word = 0;
                    if (vec) {
                        // VResizeLinearVec_32s8u (its 16-bit saturations cannot trigger
                        // for 11-bit weights, k_pyr_resize_lds)
#pragma unroll
                        for (int b = 0; b < 4; b++) {
                            const int v = (((A[b] >> 4) * b0 >> 16) + ((B[b] >> 4) * b1 >> 16) + 2) >> 2;
                            word |= (uint32_t)min(v, 255) << (8 * b);
                        }
                    } else {
#pragma unroll
                        for (int b = 0; b < 4; b++) {
                            int v;
                            if (vb[b])
                                v = (((A[b] >> 4) * b0 >> 16) + ((B[b] >> 4) * b1 >> 16) + 2) >> 2;
                            else   // FixedPtCast<int, uchar, 22>
                                v = (A[b] * b0 + B[b] * b1 + (1 << 21)) >> 22;
                            word |= (uint32_t)sat_u8(v) << (8 * b);
                        }
                    }
                    // bytes past the ROI (the last word) are overwritten by the border pass
                    *reinterpret_cast<uint32_t*>(dst + r * stride + kEdge + px0) = word;
                }
            }
        }
        CASC_MARK(l, 0);
        __syncthreads();
        CASC_MARK(l, 1);
        // 2. border columns (REFLECT_101 of the row's own pixels) and the zero
        //    tail past the padded width, per computed row
        const int tail = stride - L.pw;
        for (int i = tid; i < nrows * (2 * kEdge + tail); i += T) {
            const int r = i / (2 * kEdge + tail), k = i - r * (2 * kEdge + tail);
            uint8_t* row = dst + r * stride;
            if (k < 2 * kEdge) {
                const int px = k < kEdge ? k : L.w + k;   // 0 .. 15, then kEdge + w .. kEdge + w + 15
                row[px] = row[kEdge + reflect101(px - kEdge, L.w)];
            } else {
                row[L.pw + (k - 2 * kEdge)] = 0;
            }
        }
        __syncthreads();
        CASC_MARK(l, 2);
        // 3. the band's rows to the pyramid, 16-byte stores: its owned ROI
        //    rows, then the border rows whose reflection it owns
        {
            const int n16 = stride >> 4, nown = pl.y - pl.x;
            uint8_t* out = pyr + L.off;
            for (int i = tid; i < nown * n16; i += T) {
                const int rr = i / n16, q = i - rr * n16, r = pl.x + rr;
                *reinterpret_cast<uint4*>(out + (size_t)(kEdge + r) * stride + 16 * q) =
                    *reinterpret_cast<const uint4*>(dst + (r - c0) * stride + 16 * q);
            }
            for (int i = tid; i < 2 * kEdge * n16; i += T) {
                const int k = i / n16, q = i - k * n16;
                const int py = k < kEdge ? k : L.h + k;   // 0 .. 15, then kEdge + h .. kEdge + h + 15
                const int r = reflect101(py - kEdge, L.h);
                if (r >= pl.x && r < pl.y)
                    *reinterpret_cast<uint4*>(out + (size_t)py * stride + 16 * q) =
                        *reinterpret_cast<const uint4*>(dst + (r - c0) * stride + 16 * q);
            }
        }
        CASC_MARK(l, 3);
        if (l > 0) {
            tcol += L.w;
            trow += max(0, nrows);
        }
        // the next level reads dst's ROI bytes (final since the first barrier)
        // and writes the other buffer, which nobody reads any more
        sc0 = c0;
        sstride = stride;
    }
}

// ---------------------------------------------------------------------------
// FAST-9/16 score map.  For a pixel with value v and ring d_k = v - p_k
// (k = 0..15, OpenCV offsets), S = max(M_dark, M_bright) - 1 where M_dark is
// the best 9-arc minimum of d and M_bright that of -d.  FAST at threshold t
// classifies the pixel as a corner iff S >= t, and cornerScore<16> returns
// exactly S (OpenCV 2.4 fast.cpp / fast_score.cpp).  A pixel whose compass
// pre-test passes in one direction only has S = that direction's arc - 1.
// ---------------------------------------------------------------------------
// Two candidates per lane (a, b) on packed fp16 halves: the 8-bit pixels are
// used as they are loaded, as the fp16 subnormals p * 2^-24 (bits 0x00pp;
// the kernels run with fp16 denormals on, the compiler's default for this
// target).  Every quantity below is k * 2^-24 with |k| <= 255, so the ring
// differences d_k = v - p_k, their minima and maxima are exact and the 3-way
// windows are single v_pk_minimum3_f16 / v_pk_maximum3_f16 instructions
// (gfx950) for both candidates.  Returns r = max(dark, -bright) as bits, low
// half candidate a, high half b: a non-negative half is the integer S + 1;
// a half with its sign bit set (a negative int16) is a pixel with S < 0.
//
// The (a, b) pairs are packed by one v_lshl_or_b32 per ring point (two
// ds_read_u8): gfx950's 16-bit-half LDS loads clear the other half of the
// register, so they cannot assemble a pair.
//
// Arc reduction as OpenCV's cornerScore pairs it: with W_k = min d[k .. k+8]
// and, for even k, A_k = min d[k+1 .. k+8] (four pair minima q_j = min(d[2j+1],
// d[2j+2])), max(W_k, W_k+1) = min(A_k, max(d[k], d[k+9])): 8 + 8 + 8 + 8
// packed instructions and a 4-instruction max tree per polarity, the same
// max-of-min value as the 16 windows one by one.
typedef _Float16 orbx_h2 __attribute__((ext_vector_type(2)));
__device__ inline orbx_h2 h2_min3(orbx_h2 a, orbx_h2 b, orbx_h2 c)
{
    return __builtin_elementwise_minimum(__builtin_elementwise_minimum(a, b), c);
}
__device__ inline orbx_h2 h2_max3(orbx_h2 a, orbx_h2 b, orbx_h2 c)
{
    return __builtin_elementwise_maximum(__builtin_elementwise_maximum(a, b), c);
}
__device__ inline uint32_t fast_arc2(const uint8_t* t, int pa, int pb, int pitch)
{
    const int off[16] = {3 * pitch,      1 + 3 * pitch, 2 + 2 * pitch,  3 + pitch,
                         3,              3 - pitch,     2 - 2 * pitch,  1 - 3 * pitch,
                         -3 * pitch,     -1 - 3 * pitch, -2 - 2 * pitch, -3 - pitch,
                         -3,             -3 + pitch,    -2 + 2 * pitch, -1 + 3 * pitch};
    // bases at the ring's top-left corner: every offset is a non-negative
    // ds_read immediate (no address arithmetic per ring point)
    const int o = 3 * pitch + 3;
    int ba = pa - o, bb = pb - o;
    asm("" : "+v"(ba), "+v"(bb));   // opaque: keeps the constant offsets out of the bases
    const uint8_t* ta = t + ba;
    const uint8_t* tb = t + bb;
    auto pair = [&](int k) { return __builtin_bit_cast(orbx_h2, (uint32_t)ta[k] | ((uint32_t)tb[k] << 16)); };
    const orbx_h2 v = pair(o);
    orbx_h2 d[16];
#pragma unroll
    for (int k = 0; k < 16; k++) d[k] = v - pair(off[k] + o);
    orbx_h2 qn[8], qx[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        qn[j] = __builtin_elementwise_minimum(d[2 * j + 1], d[(2 * j + 2) & 15]);
        qx[j] = __builtin_elementwise_maximum(d[2 * j + 1], d[(2 * j + 2) & 15]);
    }
    // m[j] = max(W_2j, W_2j+1); x[j] the same for the bright arcs (min of the
    // 9-arc maxima)
    orbx_h2 m[8], x[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const orbx_h2 e0 = d[2 * j], e9 = d[(2 * j + 9) & 15];
        m[j] = h2_min3(h2_min3(qn[j], qn[(j + 1) & 7], qn[(j + 2) & 7]), qn[(j + 3) & 7],
                       __builtin_elementwise_maximum(e0, e9));
        x[j] = h2_max3(h2_max3(qx[j], qx[(j + 1) & 7], qx[(j + 2) & 7]), qx[(j + 3) & 7],
                       __builtin_elementwise_minimum(e0, e9));
    }
    // dark = max_j m[j], bright = min_j x[j] (3-way trees)
    orbx_h2 dk = h2_max3(m[0], m[1], m[2]), br = h2_min3(x[0], x[1], x[2]);
    dk = h2_max3(dk, m[3], m[4]);
    br = h2_min3(br, x[3], x[4]);
    dk = h2_max3(dk, m[5], m[6]);
    br = h2_min3(br, x[5], x[6]);
    dk = __builtin_elementwise_maximum(dk, m[7]);
    br = __builtin_elementwise_minimum(br, x[7]);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_maximum(dk, -br));
}

// One workgroup per (cell, frame).  LDS (dynamic): the cell ROI with
// 16-byte aligned rows (tile), its S' map (sm), and two bitmaps: `nz` (one
// bit per tile dword whose S' word is nonzero) and `kept` (one bit per tile
// byte that survives NMS), which reuses the tile's first bytes once the
// score pass is done (the threshold-7 rescore reloads the tile).
//  1. compass pre-test, 4 pixels per thread: a 9-arc covers two adjacent
//     compass points, so S >= tmin needs d > tmin (or < -tmin) on both;
//     survivors are compacted per wave and scored with all lanes busy; a
//     nonzero S' sets its dword's `nz` bit;
//  2. non-max suppression on the `nz` dwords only (listed with one block
//     scan), kept pixels set their `kept` bit;
//  3. raster-order compaction of the `kept` bitmap (tile byte order is
//     raster order), one block scan over ~2 bitmap words per thread.
// Where the launch has LDS to spare (plist_cap > 0), `kept` lies behind nz
// (cleared with the maps) and is followed by a list of plist_cap scored
// pixels: the score pass appends every pixel it stores, and a cell (band)
// whose pixels all fit is suppressed and emitted from that list, one lane per
// scored pixel (2 and 3 above, without nz, the dword list and the bit-serial
// loops).  A cell with more scored pixels derives nz from the S' map and
// takes the dword path.
// ---------------------------------------------------------------------------
__device__ inline int byte_of(uint32_t w, int k) { return (int)((w >> (8 * k)) & 0xFF); }

// Packed 16-bit lanes (v_pk_sub_i16 / v_pk_max_i16).
typedef short orbx_s16x2 __attribute__((ext_vector_type(2)));
__device__ inline uint32_t pk_sub16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, (orbx_s16x2)(__builtin_bit_cast(orbx_s16x2, a) - __builtin_bit_cast(orbx_s16x2, b)));
}
__device__ inline uint32_t pk_max16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t,
                              __builtin_elementwise_max(__builtin_bit_cast(orbx_s16x2, a), __builtin_bit_cast(orbx_s16x2, b)));
}
// bytes (b0, b2) or (b1, b3) of w as the packed fp16 pair (1024 + b, 1024 + b')
// (exact integers): one v_perm with the 0x64 exponent bytes from k64
__device__ inline orbx_h2 h2_bytes(uint32_t w, uint32_t k64, uint32_t sel)
{
    return __builtin_bit_cast(orbx_h2, __builtin_amdgcn_perm(k64, w, sel));
}

constexpr int kFastWideThreads = 256;   // workgroup of the wide-tile FAST instances
// Dynamic LDS of a FAST workgroup for tiles of `bytes` (host and device).
__host__ __device__ constexpr int fast_tile_bytes(int hy_max, int pitch) { return (hy_max * pitch + 511) & ~511; }
__host__ __device__ constexpr int fast_lds_bytes(int tile_bytes) { return 2 * tile_bytes + tile_bytes / 32; }
// static LDS of a 256-thread FAST workgroup: 4 survivor queues of 384
// entries (u16, or u32 for the runtime-pitch instance) + block scratch
__host__ __device__ constexpr int fast_static_lds(bool u32_entries) { return 4 * 384 * (u32_entries ? 4 : 2) + 64; }
// Extra dynamic LDS of the scored-pixel list path, behind fast_lds_bytes: the
// kept bitmap (one bit per tile byte) and the list of n entries.
__host__ __device__ constexpr int fast_list_lds(int tile_bytes, int n, bool u32_entries)
{
    return n > 0 ? tile_bytes / 8 + (((n + 1) * (u32_entries ? 4 : 2) + 15) & ~15) : 0;   // + the spare entry
}
// Default capacity of the list: the largest that the u16 prefix table and a
// cell of ~1000 scored pixels (the bench's 640x480 frames peak near that)
// need; a fuller cell takes the dword path.
constexpr int kFastListCap = 1536;
#ifndef ORBX_FAST_LDS_TARGET
#define ORBX_FAST_LDS_TARGET (40 * 1024)   // 4 workgroups per CU
#endif
constexpr int kFastLdsTarget = ORBX_FAST_LDS_TARGET;
// Diagnostic builds only (-DORBX_DIAG_REPEAT=r,b,d,f): launch resize,
// describe or FAST that many times (idempotent kernels) to price each
// stage's marginal cost inside the pipelined bench (b, once the whole-level
// blur's count, is unused).
#ifndef ORBX_DIAG_REPEAT
#define ORBX_DIAG_REPEAT 1, 1, 1, 1
#endif
constexpr int kDiagRepeat[4] = {ORBX_DIAG_REPEAT};

// kP > 0: compile-time tile pitch (>= every cell's aligned row), so ring
// offsets and row strides are immediates; kP == 0: per-cell pitch.
// kThreads: 256 for cells up to 208-byte rows; the wide tiles of large
// frames (1920x1080: 336-byte rows, 75 KB of LDS, two workgroups per CU)
// get more waves per workgroup instead.
template <int kP, int kThreads = 256, bool kBanded = false>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(kThreads > 256 ? 6 : 4))) void k_fast_cells(
    ExtractArgs a, int tile_bytes, int band_rows, int plist_cap)
{
    constexpr int kBlock = kThreads, kWaves = kThreads / 64;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ BlockScratchN<kWaves> bs;
    // Per-wave queue of compass survivors (tile positions): u16 for the
    // templated pitches (the host sends tiles over 64 KB to kP = 0), u32 for
    // kP = 0.  Linear, not a ring: after each scoring round the < 128 left
    // over move to the front, so an iteration's <= 256 new entries always fit
    // (a wave's partial last iteration is not followed by a scoring round:
    // up to 127 + 252 entries are left for the pooled pass).
    using QEntry = typename std::conditional<kP != 0, uint16_t, uint32_t>::type;
    constexpr int kQueue = 128 + 256;
    constexpr int kQueueWords = kWaves * kQueue * (int)sizeof(QEntry) / 4;
    constexpr int kUnitCap = 2 * kQueueWords;   // u16 NMS unit list aliasing the queues
    __shared__ __attribute__((aligned(16))) uint32_t qbuf[kQueueWords];
    __shared__ int s_left[kWaves];   // each wave's queue length at the end of a score pass
    uint16_t* ulist = reinterpret_cast<uint16_t*>(qbuf);
    const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    QEntry* cand = reinterpret_cast<QEntry*>(qbuf) + wv * kQueue;
    // S' (0 where not scored) and nz start at zero (contiguous: tile_bytes *
    // (1 + 1/32), a multiple of 16); kept is cleared after the score pass
    // (with a scored-pixel list, the kept bitmap behind nz is cleared too)
    const int clear16 = (tile_bytes + tile_bytes / 32 + (plist_cap > 0 ? tile_bytes / 8 : 0)) >> 4;
    // prefix of the kept bitmap's words (u16, list path), aliasing the queues
    uint16_t* kprefix = reinterpret_cast<uint16_t*>(qbuf);
    int& s_nlist = bs.vars[0];   // scored pixels of the band (may exceed plist_cap)
    const uint32_t nlist_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) int*)&s_nlist;
    auto clear_maps_at = [&](uint8_t* sm) {
        for (int i = tid; i < clear16; i += kBlock) reinterpret_cast<uint4*>(sm)[i] = make_uint4(0, 0, 0, 0);
    };
    // One cell.  tile / sm: its tile buffer and the S' map (nz follows sm).
    auto process = [&](const int cell, uint8_t* const tile, uint8_t* const sm) {
    const CellGeom C = cget(a.cells, cell);
    int32_t* count_out = a.cell_count + (size_t)f * a.ncells + cell;
    if (!C.valid) {
        if (tid == 0) *count_out = 0;
        return;
    }
    const LevelGeom L = cget(a.levels, C.level);
    const int roi_x = kEdge + C.ini_x, x_al = roi_x & ~15, sh = roi_x - x_al;
    const int hx = C.hx, hy = C.hy;
    const int nq16 = (sh + hx + 15) >> 4;               // 16-byte words loaded per row
    const int P = kP ? kP : 16 * nq16, nq = P >> 2;     // tile pitch, dwords per row
    // Level 0 may be the frame itself (level_src), where only image bytes
    // exist.  A cell's ROI starts 13 pixels inside its level (ini_x, ini_y >=
    // kEdge - 3) and ends at w - 13 (at most at w: ini_x + hx <= w and
    // ini_y + hy <= h are checked with the geometry), so the first 16-byte
    // word of a row starts at padded column x_al >= (kEdge + 13) & ~15 =
    // kEdge, image column >= 0, and the last one ends at roundup16(kEdge +
    // ini_x + hx) <= kEdge + w (w % 16 == 0), image column w; load_tile's
    // rows lie in [ini_y, ini_y + hy).  The threshold-7 rescore reloads
    // through the same load_tile.
    const LevelSrc ls = level_src(a, f, C.level, L.off, L.stride);
    const int lstride = ls.stride;
    const uint8_t* src = ls.base + (size_t)(kEdge + C.ini_y) * lstride + x_al;
    uint32_t* tile32 = reinterpret_cast<uint32_t*>(tile);
    uint32_t* sm32 = reinterpret_cast<uint32_t*>(sm);
    uint32_t* nz = reinterpret_cast<uint32_t*>(sm + tile_bytes);  // bit per tile dword
    // bit per tile byte: in the tile (after scoring), or behind nz with the list
    const bool listed = plist_cap > 0;                            // uniform over the launch
    uint32_t* kept = listed ? nz + (tile_bytes >> 7) : tile32;
    QEntry* plist = reinterpret_cast<QEntry*>(sm + tile_bytes + tile_bytes / 32 + tile_bytes / 8);
    int path_mask = 0;   // 1: a band took the list path, 2: the dword path
    FP_T0();
    // the cell's rows [w0, w0 + wh) into tile rows 0 .. wh - 1
    auto load_tile = [&](int w0, int wh) {
        uint4* t16 = reinterpret_cast<uint4*>(tile32);
        const uint8_t* src_w = src + (size_t)w0 * lstride;
        const int n = wh * nq16;
        // i / nq16 as a float product: (i + 1/2) / nq16 is at least 1/(2 nq16)
        // from an integer and the product's error is < 2^-21 (i + 1) for
        // i < 2^16, nq16 < 2^8 -- four integer divisions cost ~80 VALU
        const float inv16 = 1.0f / (float)nq16;
        auto row_of = [&](int i) { return (int)(((float)i + 0.5f) * inv16); };
        // four independent loads per round (named registers: an array here
        // was kept in scratch memory), then the LDS stores
        for (int u0 = 0; u0 < n; u0 += 4 * kBlock) {
            const int i0 = min(u0 + tid, n - 1), i1 = min(u0 + kBlock + tid, n - 1);
            const int i2 = min(u0 + 2 * kBlock + tid, n - 1), i3 = min(u0 + 3 * kBlock + tid, n - 1);
            const int r0 = row_of(i0), r1 = row_of(i1), r2 = row_of(i2), r3 = row_of(i3);
            const int c0 = i0 - r0 * nq16, c1 = i1 - r1 * nq16, c2 = i2 - r2 * nq16, c3 = i3 - r3 * nq16;
            // 32-bit offsets from the uniform tile origin (saddr loads)
            const uint4 v0 = *reinterpret_cast<const uint4*>(src_w + (uint32_t)(r0 * lstride + 16 * c0));
            const uint4 v1 = *reinterpret_cast<const uint4*>(src_w + (uint32_t)(r1 * lstride + 16 * c1));
            const uint4 v2 = *reinterpret_cast<const uint4*>(src_w + (uint32_t)(r2 * lstride + 16 * c2));
            const uint4 v3 = *reinterpret_cast<const uint4*>(src_w + (uint32_t)(r3 * lstride + 16 * c3));
            t16[r0 * (P >> 4) + c0] = v0;
            t16[r1 * (P >> 4) + c1] = v1;
            t16[r2 * (P >> 4) + c2] = v2;
            t16[r3 * (P >> 4) + c3] = v3;
        }
    };
    auto clear_maps = [&]() { clear_maps_at(sm); };
    auto clear_kept = [&]() {
        for (int i = tid; i < (tile_bytes >> 7); i += kBlock) reinterpret_cast<uint4*>(kept)[i] = make_uint4(0, 0, 0, 0);
    };
    const int c_lo = 3 + sh, c_hi = hx - 4 + sh;         // interior tile columns
    // dwords holding them; none when the ROI has no interior (hx < 7: a
    // degenerate cell of a tiny level, where c_hi < c_lo and, with a large
    // alignment shift, (c_hi >> 2) - q0 + 1 would go negative)
    const int q0 = c_lo >> 2, nqe = c_hi >= c_lo ? (c_hi >> 2) - q0 + 1 : 0;
    // pixels j >= j_lo of dword q0, j <= j_hi of the last dword q_last = q0 + nqe - 1
    const int j_lo = c_lo & 3, j_hi = c_hi & 3;
    const uint32_t k64 = 0x64646464u;
    // S' map at threshold tmin over the window rows [sr0, sr0 + nrows):
    // S' = S where S >= tmin, else 0
    auto score_pass = [&](const int tmin, const int sr0, const int nrows) {
        const int nunits = max(nrows, 0) * nqe;
        // no interior dwords (a degenerate cell of a tiny level): nothing to
        // score, and the row walk below must not divide by nqe == 0
        if (nunits <= 0) return;
        // per-wave queue cand[0, qt) of compass survivors, scored 128 at a
        // time (two per lane) with every lane busy
        auto set_nz = [&](int p) { atomicOr(&nz[p >> 7], 1u << ((p >> 2) & 31)); };
        auto score_pair = [&](int pa, int pb, bool has_a, bool has_b) {
            if (!has_a) return;
            // S + 1 from the bit pattern (a set sign bit: a negative int16)
            const uint32_t rb = fast_arc2(tile, pa, pb, P);
            const int Sa = (int)(int16_t)rb - 1, Sb = ((int32_t)rb >> 16) - 1;
            const bool st_a = Sa >= tmin, st_b = has_b && Sb >= tmin;
            if (listed) {
                // the stored pixels join the band's list: one LDS atomic per
                // batch (by the first lane that stores; the compiler's own
                // wave aggregation of atomicAdd cost 20 more instructions),
                // slots by lane rank (a's, then b's); entries past the
                // capacity go to the spare entry behind it, the count goes on
                const uint64_t ma = __builtin_amdgcn_ballot_w64(st_a), mb = __builtin_amdgcn_ballot_w64(st_b);
                const uint32_t na = (uint32_t)__popcll(ma), nab = na + (uint32_t)__popcll(mb);
                uint32_t base = 0;
                if (nab) {   // uniform
                    const uint32_t first = (uint32_t)__builtin_ctzll(ma | mb);
                    uint64_t saved;
                    uint32_t ret;
                    asm volatile("s_mov_b64 %0, exec\n\t"
                                 "s_mov_b64 exec, %2\n\tds_add_rtn_u32 %1, %3, %4\n\t"
                                 "s_mov_b64 exec, %0\n\ts_waitcnt lgkmcnt(0)"
                                 : "=&s"(saved), "=&v"(ret)
                                 : "s"(1ull << first), "v"(nlist_lds), "v"(nab)
                                 : "memory");
                    base = (uint32_t)__builtin_amdgcn_readlane((int)ret, (int)first);
#ifdef ORBX_FAST_PROFILE
                    if (lane == first) FP_ADD(19, nab);
#endif
                }
                const uint32_t ia = __builtin_amdgcn_mbcnt_hi((uint32_t)(ma >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ma, base));
                const uint32_t ib =
                    __builtin_amdgcn_mbcnt_hi((uint32_t)(mb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mb, base + na));
                if (st_a) {
                    sm[pa] = (uint8_t)Sa;
                    plist[min(ia, (uint32_t)plist_cap)] = (QEntry)pa;
                }
                if (st_b) {
                    sm[pb] = (uint8_t)Sb;
                    plist[min(ib, (uint32_t)plist_cap)] = (QEntry)pb;
                }
            } else {
                if (st_a) {
                    sm[pa] = (uint8_t)Sa;
                    set_nz(pa);
                }
                if (st_b) {
                    sm[pb] = (uint8_t)Sb;
                    set_nz(pb);
                }
            }
        };
        // pass <=> max(v - A, B - v) >= tmin + 1 with A = min of the four
        // adjacent compass-pair maxima, B = max of the pair minima (exact
        // on the fp16 integers 1024 + p; the sign bit of the difference
        // is clear exactly when the test passes)
        const orbx_h2 T1 = {(_Float16)(tmin + 1), (_Float16)(tmin + 1)};
        // Pixel j of dword q0 lies outside the interior columns when j < j_lo,
        // of dword q_last when j > j_hi: uniform all-or-nothing masks, AND-ed
        // with the lane masks of the two dwords.
        // (opaque scalar pairs: else each use is rebuilt as a compare and
        // two selects inside the loop)
        auto cut_mask = [](bool c) {
            const uint32_t m = __builtin_amdgcn_readfirstlane(c ? ~0u : 0u);
            uint64_t r = ((uint64_t)m << 32) | m;
            asm("" : "+s"(r));
            return r;
        };
        const uint64_t cutA0 = cut_mask(j_lo > 0), cutA1 = cut_mask(j_lo > 1), cutA2 = cut_mask(j_lo > 2);
        const uint64_t cutB1 = cut_mask(j_hi < 1), cutB2 = cut_mask(j_hi < 2), cutB3 = cut_mask(j_hi < 3);
        // the wave's queue as a uniform LDS byte address, and the address of
        // its end (cand[qt]), which the loop keeps in place of qt
        typedef __attribute__((address_space(3))) QEntry LdsEntry;
        const uint32_t cand_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(LdsEntry*)cand);
        constexpr int kEsh = sizeof(QEntry) == 2 ? 1 : 2;   // log2 of an entry's bytes
        uint32_t qe = cand_lds;
        // One compass unit per lane: the tile dword at byte offset `pos` (4
        // pixels), whose interior dword number in its row is qr (0 .. nqe - 1).
        // Survivors of the lanes in `live` are appended to the queue in
        // plane-major order.
        auto compass = [&](const int pos, const int qr, const uint64_t live) {
            const uint32_t* row = reinterpret_cast<const uint32_t*>(tile + pos);
            const uint32_t mid = row[0];
            // row[-1] / row[1] past the row ends are the neighbouring rows'
            // dwords (an interior row): only pixels outside the interior
            // columns read them, and those are masked below
            const uint32_t lo = row[-1], hi = row[1];
            const uint32_t up = row[-3 * nq], dn = row[3 * nq];
            // 4 pixels at once: even / odd bytes as two packed fp16 halves
            const uint32_t p4w = __builtin_amdgcn_alignbyte(hi, mid, 3);    // bytes j+3
            const uint32_t p12w = __builtin_amdgcn_alignbyte(mid, lo, 1);   // bytes j-3
            // per pixel j: the sign bit of x_j = max(v - A, B - v) - tmin - 1
            // is set where the pixel fails (even half: j = 0, 2; odd: 1, 3)
            uint32_t xw[2];
#pragma unroll
            for (int hf = 0; hf < 2; hf++) {
                const uint32_t sel = hf ? 0x04030401u : 0x04020400u;   // bytes 1,3 or 0,2 | 0x64
                const orbx_h2 v = h2_bytes(mid, k64, sel);
                // compass points in ring order 0, 4, 8, 12
                const orbx_h2 p0 = h2_bytes(dn, k64, sel), p4 = h2_bytes(p4w, k64, sel);
                const orbx_h2 p8 = h2_bytes(up, k64, sel), p12 = h2_bytes(p12w, k64, sel);
                // IEEE maximum / minimum: no canonicalising moves (the
                // operands are finite).  A = min over the adjacent pairs
                // (0,4), (4,8), (8,12), (12,0) of the pair maximum; by
                // distributivity min(max(a, x), max(b, x)) = max(x, min(a, b))
                // that is max(min(p4, p12), min(p0, p8)); likewise
                // B = max over the pairs of the pair minimum
                // = min(max(p4, p12), max(p0, p8)).
                const orbx_h2 A = __builtin_elementwise_maximum(__builtin_elementwise_minimum(p4, p12),
                                                                __builtin_elementwise_minimum(p0, p8));
                const orbx_h2 B = __builtin_elementwise_minimum(__builtin_elementwise_maximum(p4, p12),
                                                                __builtin_elementwise_maximum(p0, p8));
                const orbx_h2 x = __builtin_elementwise_maximum(v - A, B - v) - T1;
                xw[hf] = __builtin_bit_cast(uint32_t, x);
            }
            // pass flags as lane masks straight from the compares (bit 15 /
            // 31 clear: a 16-bit and a 32-bit signed compare each; low halves
            // as fp16 >= 0: no -0 or NaN arises from these exact integer
            // differences); the cuts and `live` are 64-bit scalar operations
            const uint64_t at0 = __builtin_amdgcn_ballot_w64(qr == 0), atl = __builtin_amdgcn_ballot_w64(qr == nqe - 1);
            const uint64_t b0 = __builtin_amdgcn_ballot_w64(__builtin_bit_cast(orbx_h2, xw[0]).x >= (_Float16)0) &
                                ~(at0 & cutA0) & live;
            const uint64_t b1 = __builtin_amdgcn_ballot_w64(__builtin_bit_cast(orbx_h2, xw[1]).x >= (_Float16)0) &
                                ~((at0 & cutA1) | (atl & cutB1)) & live;
            const uint64_t b2 = __builtin_amdgcn_ballot_w64((int32_t)xw[0] >= 0) & ~((at0 & cutA2) | (atl & cutB2)) & live;
            const uint64_t b3 = __builtin_amdgcn_ballot_w64((int32_t)xw[1] >= 0) & ~(atl & cutB3) & live;
            const int n0 = __popcll(b0), n1 = __popcll(b1), n2 = __popcll(b2), n3 = __popcll(b3);
            // plane-major order: each plane's survivors at their lane rank
            // after the earlier planes'; the plane's start is part of the
            // scalar base of the address (opaque: the compiler would move it
            // into a vector add per plane)
            auto slot = [&](uint64_t bm, uint32_t base) {
                asm("" : "+s"(base));
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
                return (rank << kEsh) + base;
            };
            const uint32_t s1 = qe + ((uint32_t)n0 << kEsh), s2 = s1 + ((uint32_t)n1 << kEsh);
            const uint32_t s3 = s2 + ((uint32_t)n2 << kEsh);
            const uint32_t a0 = slot(b0, qe), a1 = slot(b1, s1), a2 = slot(b2, s2), a3 = slot(b3, s3);
            const uint32_t e0 = (uint32_t)pos, e1 = e0 | 1u, e2 = e0 | 2u, e3 = e0 | 3u;
            // the four stores under their planes' lane masks, with one save
            // and one restore of exec (as `if (pass_j) queue[slot_j] = e_j`
            // the compiler wraps each store in an exec region with a branch).
            // LDS operations of a wave complete in order, so the queue reads
            // below see these stores; the compiler's lgkmcnt waits do not
            // count them, which only makes a later wait conservative.
            uint64_t saved;
            if constexpr (sizeof(QEntry) == 2)
                asm volatile("s_mov_b64 %0, exec\n\t"
                             "s_mov_b64 exec, %1\n\tds_write_b16 %5, %9\n\t"
                             "s_mov_b64 exec, %2\n\tds_write_b16 %6, %10\n\t"
                             "s_mov_b64 exec, %3\n\tds_write_b16 %7, %11\n\t"
                             "s_mov_b64 exec, %4\n\tds_write_b16 %8, %12\n\t"
                             "s_mov_b64 exec, %0"
                             : "=&s"(saved)
                             : "s"(b0), "s"(b1), "s"(b2), "s"(b3), "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(e0), "v"(e1),
                               "v"(e2), "v"(e3)
                             : "memory");
            else
                asm volatile("s_mov_b64 %0, exec\n\t"
                             "s_mov_b64 exec, %1\n\tds_write_b32 %5, %9\n\t"
                             "s_mov_b64 exec, %2\n\tds_write_b32 %6, %10\n\t"
                             "s_mov_b64 exec, %3\n\tds_write_b32 %7, %11\n\t"
                             "s_mov_b64 exec, %4\n\tds_write_b32 %8, %12\n\t"
                             "s_mov_b64 exec, %0"
                             : "=&s"(saved)
                             : "s"(b0), "s"(b1), "s"(b2), "s"(b3), "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(e0), "v"(e1),
                               "v"(e2), "v"(e3)
                             : "memory");
            qe = __builtin_amdgcn_readfirstlane(s3 + ((uint32_t)n3 << kEsh));   // wave-uniform
#ifdef ORBX_FAST_PROFILE
            if (lane == 0) FP_ADD(10 + (tmin < 10), n0 + n1 + n2 + n3);
            if (lane == 0) FP_ADD(12, 1);
#endif
        };
        // The lane's unit u = u0 + lane as (tile dword, dword number in its
        // row), kept incrementally: a step of kBlock units is dr rows and dq
        // dwords, with at most one wrap into the next row (dq < nqe).  nqe
        // ranges from 1 (dq = 0: never wraps) to more than kBlock (dr = 0).
        const int wvu = __builtin_amdgcn_readfirstlane(wv);   // the loop count is wave-uniform
        const int start = wvu * 64 + lane, row0 = start / nqe;
        uint32_t qr = start - row0 * nqe;
        int pos = 4 * ((sr0 + row0) * nq + q0 + (int)qr);
        const int dr = kBlock / nqe, dq = kBlock - dr * nqe;
        const int step = 4 * (dr * nq + dq);
        int wrap_pos = 4 * (nq - nqe);
        asm("" : "+v"(wrap_pos));   // a register operand of the select below
        int u0 = wvu * 64;
        // full iterations (every lane has a unit), then at most one partial
        // one, the wave's last
        for (; u0 + 64 <= nunits; u0 += kBlock) {
            compass(pos, (int)qr, ~0ull);
            // qr + dq < 2 nqe: where it reaches nqe the unsigned minimum picks
            // the wrapped value (else qr - nqe is huge)
            qr += dq;
            const uint32_t qw = qr - (uint32_t)nqe;
            pos += step + ((int32_t)qw >= 0 ? wrap_pos : 0);
            qr = min(qr, qw);
            if (qe - cand_lds >= (128u << kEsh)) {   // uniform: score full batches, move the rest to the front
                const int qt = (int)((qe - cand_lds) >> kEsh);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                int qh = 0;
                for (; qt - qh >= 128; qh += 128) {
#ifdef ORBX_FAST_PROFILE
                    if (lane == 0) FP_ADD(13, 1);
#endif
                    score_pair(cand[qh + lane], cand[qh + 64 + lane], true, true);
                }
                const int rest = qt - qh;   // < 128
                const QEntry e0 = lane < rest ? cand[qh + lane] : (QEntry)0;
                const QEntry e1 = lane + 64 < rest ? cand[qh + 64 + lane] : (QEntry)0;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (lane < rest) cand[lane] = e0;
                if (lane + 64 < rest) cand[lane + 64] = e1;
                qe = cand_lds + ((uint32_t)__builtin_amdgcn_readfirstlane(rest) << kEsh);
            }
            // no fence here: the next iteration appends at >= qt (the moved
            // rest lies below it), and the queue is read only after the
            // fence above
        }
        if (u0 < nunits) {
            // lanes past the last unit read lane 0's dwords (inside the tile)
            // and append nothing; the queue then holds < 128 + 256 entries,
            // all scored with the leftovers below
            const int rem = nunits - u0;   // 1 .. 63
            const int pos0 = __builtin_amdgcn_readfirstlane(pos);
            compass(lane < rem ? pos : pos0, (int)qr, (1ull << rem) - 1);
        }
        // the waves' leftovers (< kQueue each) scored together, in full batches
        // of 128 where they add up (one partly filled batch per wave would
        // run the whole scoring code for a few pixels)
        if (lane == 0) s_left[wv] = (int)((qe - cand_lds) >> kEsh);
        __syncthreads();
        int pre[kWaves + 1];
        pre[0] = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) pre[w + 1] = pre[w] + s_left[w];
        const int T = pre[kWaves];
        auto entry = [&](int g) {
            int w = 0;
#pragma unroll
            for (int k = 1; k < kWaves; k++) w += g >= pre[k];
            return (int)(reinterpret_cast<const QEntry*>(qbuf) + w * kQueue)[g - pre[w]];
        };
        for (int b0 = wv * 128; b0 < T; b0 += kWaves * 128) {
            const int ga = b0 + lane, gb = b0 + 64 + lane;
#ifdef ORBX_FAST_PROFILE
            if (lane == 0) FP_ADD(14, 1);
            if (lane == 0) FP_ADD(15, min(128, T - b0));
#endif
            score_pair(ga < T ? entry(ga) : 0, gb < T ? entry(gb) : 0, ga < T, gb < T);
        }
    };
    // non-max suppression over the S' map: a pixel is kept if its S' beats
    // all 8 neighbours' S'.  Only dwords whose `nz` bit is set can keep
    // anything; they are listed (u16 tile dword indices, in windows of
    // kUnitCap) with one block scan and shared by all 256 threads.
    // Only the window rows [rb0, rb1) (the band's own rows) keep anything;
    // the halo rows' S' serve as their neighbours.
    // Returns this thread's count of kept corners at fastTh.
    auto nms_pass = [&](const int rb0, const int rb1, const int wh) {
        int c1 = 0;
        const uint32_t FT = (uint32_t)max(a.fast_th, 1) * 0x00010001u;
        auto nms_unit = [&](int idx) {
            const int rw = idx / nq, q = idx - rw * nq;
            if (rw < rb0 || rw >= rb1) return;
            const uint32_t* m = sm32 + idx;
            const uint32_t mid = m[0];
            // the 8 neighbours of the 4 pixels as dwords (bytes j-1, j, j+1 of
            // rows r-1, r, r+1), byte-wise max on even / odd u16x2 halves
            uint32_t nb[8];
            int k = 0;
#pragma unroll
            for (int dr = 0; dr < 3; dr++) {
                const uint32_t* mr = m + (dr - 1) * nq;
                const uint32_t lo = q > 0 ? mr[-1] : 0u, mm = mr[0], hi = q + 1 < nq ? mr[1] : 0u;
                nb[k++] = __builtin_amdgcn_alignbyte(mm, lo, 3);   // j-1
                if (dr != 1) nb[k++] = mm;
                nb[k++] = __builtin_amdgcn_alignbyte(hi, mm, 1);   // j+1
            }
            uint32_t bits = 0;
#pragma unroll
            for (int hf = 0; hf < 2; hf++) {
                const uint32_t sel = hf ? 0x0c030c01u : 0x0c020c00u;
                uint32_t mx = __builtin_amdgcn_perm(0u, nb[0], sel);
#pragma unroll
                for (int i = 1; i < 8; i++) mx = pk_max16(mx, __builtin_amdgcn_perm(0u, nb[i], sel));
                const uint32_t sv = __builtin_amdgcn_perm(0u, mid, sel);
                // keep where mx - s < 0 (s > every neighbour)
                const uint32_t keep = pk_sub16(mx, sv) & 0x80008000u;
                // pixel j -> bit j (even half: j = 0, 2; odd half: j = 1, 3)
                bits |= ((keep >> 15) & 1) << hf | ((keep >> 31) & 1) << (2 + hf);
                // corners at fastTh among the kept (kept >= max(fastTh, 1))
                const uint32_t kept16 = sv & ((keep >> 15) * 0xFFFFu);
                c1 += __popc(~pk_sub16(kept16, FT) & keep);
            }
            if (bits) atomicOr(&kept[idx >> 3], bits << (4 * (idx & 7)));
        };
        const int nw = (wh * nq + 31) >> 5;                  // nz words
        const int pw = (nw + kBlock - 1) / kBlock;
        const int w0 = min(tid * pw, nw), w1 = min(w0 + pw, nw);
        int cnt = 0;
        for (int w = w0; w < w1; w++) cnt += __popc(nz[w]);
        int total;
        const int off0 = block_exclusive_scan(cnt, &total, bs, 1);
        for (int base = 0; base < total; base += kUnitCap) {
            if (base > 0) __syncthreads();                   // previous window consumed
            if (cnt && off0 < base + kUnitCap && off0 + cnt > base) {
                int off = off0;
                for (int w = w0; w < w1; w++) {
                    uint32_t b = nz[w];
                    while (b) {
                        const int bit = __builtin_ctz(b);
                        b &= b - 1;
                        if (off >= base && off < base + kUnitCap) ulist[off - base] = (uint16_t)(32 * w + bit);
                        off++;
                    }
                }
            }
            __syncthreads();
            const int n = min(total - base, kUnitCap);
#ifdef ORBX_FAST_PROFILE
            if (tid == 0) FP_ADD(16, n);
            if (tid == 0) FP_ADD(17, (n + kBlock - 1) / kBlock);
#endif
            for (int i = tid; i < n; i += kBlock) nms_unit((int)ulist[i]);
        }
        return c1;
    };
    // The same from the band's list of scored pixels (n <= plist_cap of them,
    // in any order), one per lane: S' against the map's eight neighbour bytes
    // (0 where not scored; a scored pixel is an interior one, so all eight
    // lie in its tile rows' neighbours).
    bool on_list = false;   // the current band's path
    auto nms_list = [&](const int rb0, const int rb1, const int n) {
        int c1 = 0;
        const int ft = max(a.fast_th, 1);
        for (int i = tid; i < n; i += kBlock) {
            const int pos = (int)plist[i];
            const uint8_t* m = sm + pos;
            const uint32_t s = m[0];
            const uint32_t up = max(max((uint32_t)m[-P - 1], (uint32_t)m[-P]), (uint32_t)m[-P + 1]);
            const uint32_t dn = max(max((uint32_t)m[P - 1], (uint32_t)m[P]), (uint32_t)m[P + 1]);
            bool keep = s > max(max(up, dn), max((uint32_t)m[-1], (uint32_t)m[1]));
            if constexpr (kBanded) {   // halo rows are scored, not kept
                const int rw = pos / P;
                keep = keep && rw >= rb0 && rw < rb1;
            }
            if (keep) {
                atomicOr(&kept[pos >> 5], 1u << (pos & 31));
                c1 += (int)s >= ft;
            }
        }
#ifdef ORBX_FAST_PROFILE
        if (tid == 0) FP_ADD(20, (n + kBlock - 1) / kBlock);
        if (tid == 0) atomicMax(&g_fast_prof[21], (unsigned long long)n);
#endif
        return c1;
    };
    // The dword path's nz bitmap from the S' map (a band whose scored pixels
    // overflowed the list): each wave's 64 dwords are two nz words.
    auto nz_from_map = [&]() {
        for (int i = tid; i < (tile_bytes >> 2); i += kBlock) {   // tile_bytes / 4 is a multiple of 128
            const uint64_t b = __builtin_amdgcn_ballot_w64(sm32[i] != 0);
            if (lane == 0) *reinterpret_cast<uint64_t*>(&nz[i >> 5]) = b;
        }
    };
    uint32_t* out = a.cell_lists + (size_t)f * a.list_entries + C.list_off;
    // The list path's emission into the cell's list at out_base (t, tmin and
    // the return value as compact's, below): a kept pixel's raster rank is
    // the prefix of its bitmap word (one block scan, written to LDS) plus the
    // kept bits below it in the word; each listed pixel's lane writes its own
    // entry.
    auto emit_list = [&](const int t, const int tmin, const int w0, const int wh, const int out_base) {
        const int n = s_nlist;
        if (t != tmin) {   // fastTh < 7 fell back to 7: only S' >= t is emitted, and ranked
            for (int i = tid; i < n; i += kBlock) {
                const int pos = (int)plist[i];
                if (sm[pos] < t) atomicAnd(&kept[pos >> 5], ~(1u << (pos & 31)));
            }
            __syncthreads();
        }
        const int nkw = (wh * P + 31) >> 5;
        const int per = (nkw + kBlock - 1) / kBlock;
        const int ka = min(tid * per, nkw), kb = min(ka + per, nkw);
        int cnt = 0;
        for (int k = ka; k < kb; k++) cnt += __popc(kept[k]);
        int total;
        int off = block_exclusive_scan(cnt, &total, bs, 1);
        for (int k = ka; k < kb; k++) {
            kprefix[k] = (uint16_t)off;
            off += __popc(kept[k]);
        }
        __syncthreads();
        for (int i = tid; i < n; i += kBlock) {
            const int pos = (int)plist[i];
            const uint32_t w = kept[pos >> 5], bit = 1u << (pos & 31);
            if (w & bit) {
                const int o = out_base + (int)kprefix[pos >> 5] + __popc(w & (bit - 1));
                if (o < C.list_cap) {
                    const int r = w0 + pos / P, cc = pos % P - sh;   // cell row, ROI column
                    out[o] = ((uint32_t)sm[pos] << 24) | ((uint32_t)(C.ini_y + r) << 12) | (uint32_t)(C.ini_x + cc);
                }
            }
        }
#ifdef ORBX_FAST_PROFILE
        if (tid == 0) FP_ADD(22, total);
        if (tid == 0) atomicMax(&g_fast_prof[23], (unsigned long long)total);
#endif
        return total;
    };
    // Raster-order compaction of the kept bitmap into the cell's list at
    // out_base: thread tid owns the contiguous bitmap words [ka, kb); kept
    // bytes are S' >= tmin of the pass, and t == tmin unless fastTh < 7 fell
    // back to 7 (then each byte is compared).  Returns the entries written.
    // (A band on the list path: emit_list.)
    auto compact = [&](const int t, const int tmin, const int w0, const int wh, const int out_base) {
        if (on_list) return emit_list(t, tmin, w0, wh, out_base);
        const int nkw = (wh * P + 31) >> 5;
        const int per = (nkw + kBlock - 1) / kBlock;
        const int ka = min(tid * per, nkw), kb = min(ka + per, nkw);
        const bool all_kept = t == tmin;
#ifdef ORBX_FAST_PROFILE
        if (tid == 0) FP_ADD(18, per);
#endif
        int cnt = 0;
        for (int k = ka; k < kb; k++) {
            uint32_t b = kept[k];
            if (all_kept) {
                cnt += __popc(b);
            } else {
                while (b) {
                    const int bit = __builtin_ctz(b);
                    b &= b - 1;
                    cnt += sm[32 * k + bit] >= t;
                }
            }
        }
        int total;
        int off = out_base + block_exclusive_scan(cnt, &total, bs, 1);
        if (cnt) {
            // entries go straight to the cell's list (each thread's run is
            // contiguous; the tile area holds the kept bitmap being read)
            for (int k = ka; k < kb; k++) {
                uint32_t b = kept[k];
                while (b) {
                    const int bit = __builtin_ctz(b);
                    b &= b - 1;
                    const int pos = 32 * k + bit;
                    const int s = sm[pos];
                    if (s >= t) {
                        if (off < C.list_cap) {
                            const int r = w0 + pos / P, cc = pos % P - sh;   // cell row, ROI column
                            out[off] = ((uint32_t)s << 24) | ((uint32_t)(C.ini_y + r) << 12) | (uint32_t)(C.ini_x + cc);
                        }
                        off++;
                    }
                }
            }
        }
        return total;
    };
    // One band: the cell rows [b0, b1) (interior rows 3 .. hy - 4).  Its
    // window holds the rows [b0 - 4, b1 + 4) (clipped to the cell): FAST's
    // 3-pixel radius around the rows b0 - 1 .. b1 whose S' the band's NMS
    // reads.  Scores, suppresses and (emit) appends the band's kept corners
    // at out_base; returns the band's kept corners at fastTh.  A whole cell
    // is one band unless the host splits tall cells (band_rows) so that a
    // workgroup's LDS stays small (1920x1080: 4 workgroups per CU instead of
    // 2); S' of a row depends only on the rows within 3 of it, so the split
    // is exact.
    auto band = [&](const int b0, const int b1, const int tmin, const bool loaded = false) {
        const int w0 = max(0, b0 - 4), wh = min(hy, b1 + 4) - w0;
        const int s0 = max(3, b0 - 1), s1 = min(hy - 4, b1);   // scored rows (inclusive)
        if (!loaded) {
            FP_MARK(7);
            load_tile(w0, wh);
            FP_MARK(5);
            clear_maps();
            if (tid == 0) s_nlist = 0;
            FP_MARK(6);
            __syncthreads();
        }
        FP_MARK(0);
        score_pass(tmin, s0 - w0, s1 - s0 + 1);
        __syncthreads();
        FP_MARK(1);
        int c1;
        on_list = listed && s_nlist <= plist_cap;   // uniform over the block
        if (on_list) {
            c1 = nms_list(b0 - w0, b1 - w0, s_nlist);
        } else {
            if (listed) nz_from_map();   // kept is clear already
            else clear_kept();           // the tile is dead until the next band reloads it
            __syncthreads();
            c1 = nms_pass(b0 - w0, b1 - w0, wh);
        }
        path_mask |= on_list ? 1 : 2;
        if (tid == 0) FP_ADD(on_list ? 24 : 25, 1);
        // (its barrier also ends the kept bitmap's updates)
        const int n1 = block_sum(c1, bs, 0);
        // (the list path's next steps touch nothing that a thread still
        // before this point reads: s_nlist, the list and S' were read before
        // block_sum's barrier)
        if (!on_list) __syncthreads();
        return n1;
    };
    // Thresholds (:599-614): FAST(fastTh), and FAST(7) when that finds <= 3
    // corners.  The S' map at threshold t gives both answers for t <= min
    // (NMS against S' equals NMS against the t-score map for corners >= t),
    // so a cell is scored at fastTh first (far fewer compass survivors) and
    // rescored at 7 only when it needs the fallback.
    int n1 = 0, written = 0;
    if constexpr (kBanded) {
        // each band is emitted at fastTh as it is done; a cell whose kept
        // corners at fastTh number <= 3 is scored again band by band (at 7,
        // or at fastTh < 7 and filtered to >= 7) and re-emitted
        const int brows = band_rows > 0 ? band_rows : hy;
        for (int b0 = 3; b0 < hy - 3; b0 += brows) {
            const int b1 = min(b0 + brows, hy - 3);
            n1 += band(b0, b1, a.fast_th);
            written += compact(a.fast_th, a.fast_th, max(0, b0 - 4), min(hy, b1 + 4) - max(0, b0 - 4), written);
            __syncthreads();   // kept / S' reused by the next band
        }
        if (n1 <= 3) {   // uniform over the block
            const int tmin2 = a.fast_th > a.fast_th_low ? a.fast_th_low : a.fast_th;
            written = 0;
            for (int b0 = 3; b0 < hy - 3; b0 += brows) {
                const int b1 = min(b0 + brows, hy - 3);
                band(b0, b1, tmin2);
                written += compact(a.fast_th_low, tmin2, max(0, b0 - 4), min(hy, b1 + 4) - max(0, b0 - 4), written);
                __syncthreads();
            }
        }
    } else if (hy > 6) {   // the whole cell as one band (the host sends band_rows = 0)
        int tmin_final = a.fast_th;
        n1 = band(3, hy - 3, a.fast_th);
        FP_MARK(2);
        if (a.fast_th > a.fast_th_low && n1 <= 3) {   // uniform over the block
            if (threadIdx.x == 0) FP_ADD(8, 1);
            tmin_final = a.fast_th_low;
            band(3, hy - 3, a.fast_th_low);
            FP_MARK(3);
        }
        // threshold choice: FAST(fastTh); if <= 3 corners, FAST(7) (:607-614)
        written = compact(n1 <= 3 ? a.fast_th_low : a.fast_th, tmin_final, 0, hy, 0);
    }
    if (tid == 0) {
        *count_out = written;
        a.fast_path[(size_t)(a.first_slot + f) * a.ncells + cell] = (uint8_t)path_mask;
        if (written > C.list_cap) atomicOr(a.error_flags, 1);
    }
    FP_MARK(4);
    if (tid == 0) FP_ADD(9, 1);
    };
    process(blockIdx.x, smem, smem + tile_bytes);
}

// ---------------------------------------------------------------------------
// retainBest, in two launches (src/ORBextractor.cc:622-701):
//  k_retain_cells   one wave per (cell, frame): the level's quota
//                   redistribution (:622-670, wave-parallel over cells),
//                   nth_element of the cell list (:683-685; in registers
//                   up to 64 corners and once the range is down to 64, in
//                   a wave-private LDS buffer before that, in global memory
//                   beyond kRetainCellCap), and the retained prefix written to
//                   the cell's slot of the level list (cell order, :687-694);
//  k_retain_levels  one wave per (level, frame): nth_element of the level
//                   list when it exceeds the level quota (:697-701).
// ---------------------------------------------------------------------------
__device__ inline void level_quota(const ExtractArgs& a, const LevelGeom& L, const int32_t* counts, int cell,
                                   int* keep_c, int* pre_c, int* level_total)
{
    const int lane = threadIdx.x & 63;
    const int nCells = L.n_cells, nfc = L.nfeatures_cell;
    constexpr int kPer = 4;   // cells per lane (<= 256 cells per level)
    int tot[kPer], ret[kPer];
    bool nomore[kPer];
    int toDist = 0, nNoMore = 0;
    // slots past the level's cells are skipped (a uniform branch): C2's
    // levels have <= 30 cells, so one slot of 64 does all the work
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int c = lane + 64 * k;
        tot[k] = 0;
        ret[k] = 0;
        nomore[k] = false;
        if (64 * k < nCells && c < nCells) {
            tot[k] = counts[c];
            if (a.cells[L.cell_base + c].valid) {
                if (tot[k] > nfc) {
                    ret[k] = nfc;
                } else {
                    ret[k] = tot[k];
                    toDist += nfc - tot[k];
                    nomore[k] = true;
                    nNoMore++;
                }
            }
        }
    }
    toDist = wave_sum(toDist);
    nNoMore = wave_sum(nNoMore);
    while (toDist > 0 && nNoMore < nCells) {
        const int nNew = nfc + (int)ceilf(__fdiv_rn((float)toDist, (float)(nCells - nNoMore)));
        int td = 0, nm = 0;
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            if (64 * k >= nCells) break;
            const int c = lane + 64 * k;
            if (c < nCells && !nomore[k]) {
                if (tot[k] > nNew) {
                    ret[k] = nNew;
                } else {
                    ret[k] = tot[k];
                    td += nNew - tot[k];
                    nomore[k] = true;
                    nm++;
                }
            }
        }
        toDist = wave_sum(td);
        nNoMore += wave_sum(nm);
    }
    int base = 0, my_keep = 0, my_pre = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if (64 * k >= nCells) break;
        const int c = lane + 64 * k;
        const int take = (c < nCells && tot[k] > 0 && ret[k] > 0) ? min(tot[k], ret[k]) : 0;
        const int incl = wave_inclusive_scan(take);
        const int kk = __builtin_amdgcn_readlane(ret[k], cell & 63), pp = __builtin_amdgcn_readlane(base + incl - take, cell & 63);
        if ((cell >> 6) == k) {
            my_keep = kk;
            my_pre = pp;
        }
        base += __builtin_amdgcn_readlane(incl, 63);
    }
    *keep_c = my_keep;
    *pre_c = my_pre;
    *level_total = base;
}

// ---------------------------------------------------------------------------
// HarrisResponses(cellImage, cellKeyPoints, 7, HARRIS_K) (:79-120, :616-620)
// on each cell's FAST list, one thread per corner: the 7x7 block of 3x3
// Sobel products around the corner (9x9 pixels of the unblurred level,
// three rows live in registers), integer sums, then the float response in
// the source's evaluation order with every operation rounded on its own
// (no contraction).  The entry becomes harris_key(response) << 32 | y << 12
// | x, so the retain kernels compare responses exactly as retainBest does.
// ---------------------------------------------------------------------------
constexpr float kHarrisK = 0.04f;                                  // HARRIS_K (:73)
constexpr float kHarrisScale = 1.0f / ((1 << 2) * 7 * 255.0f);     // 1 / ((1<<2) blockSize 255)  (:90-91)
constexpr float kHarrisScale4 = kHarrisScale * kHarrisScale * kHarrisScale * kHarrisScale;   // (:92)

__global__ __launch_bounds__(256) void k_harris_cells(ExtractArgs a)
{
    const int cell = blockIdx.x, f = blockIdx.y;
    const CellGeom C = cget(a.cells, cell);
    if (!C.valid) return;
    const int n = min(a.cell_count[(size_t)f * a.ncells + cell], C.list_cap);
    const LevelGeom L = cget(a.levels, C.level);
    // 9x9 windows around corners at least 16 pixels inside the level: image
    // pixels only (level 0 may be the frame itself, level_src)
    const LevelSrc ls = level_src(a, f, C.level, L.off, L.stride);
    const int stride = ls.stride;
    const uint8_t* img = ls.base + (size_t)kEdge * stride + kEdge;
    const uint32_t* src = a.cell_lists + (size_t)f * a.list_entries + C.list_off;
    uint64_t* dst = a.cell_keys64 + (size_t)f * a.list_entries + C.list_off;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t e = src[i];
        const int y = (int)((e >> 12) & 0xFFF), x = (int)(e & 0xFFF);
        const uint8_t* p0 = img + (ptrdiff_t)(y - 4) * stride + (x - 4);
        int r0[9], r1[9], r2[9];
#pragma unroll
        for (int j = 0; j < 9; j++) {
            r0[j] = p0[j];
            r1[j] = p0[stride + j];
        }
        int sa = 0, sb = 0, sc = 0;
#pragma unroll
        for (int rr = 2; rr < 9; rr++) {
#pragma unroll
            for (int j = 0; j < 9; j++) r2[j] = p0[(ptrdiff_t)rr * stride + j];
#pragma unroll
            for (int j = 1; j < 8; j++) {
                const int Ix = (r1[j + 1] - r1[j - 1]) * 2 + (r0[j + 1] - r0[j - 1]) + (r2[j + 1] - r2[j - 1]);
                const int Iy = (r2[j] - r0[j]) * 2 + (r2[j - 1] - r0[j - 1]) + (r2[j + 1] - r0[j + 1]);
                sa += Ix * Ix;
                sb += Iy * Iy;
                sc += Ix * Iy;
            }
#pragma unroll
            for (int j = 0; j < 9; j++) {
                r0[j] = r1[j];
                r1[j] = r2[j];
            }
        }
        const float fa = (float)sa, fb = (float)sb, fc = (float)sc;
        const float s2 = __fadd_rn(fa, fb);
        // (a*b - c*c) - (k*(a+b))*(a+b), each operation rounded (ISO), or as
        // GCC contracts it on an FMA host: fma(a, b, -(c*c)), then
        // fma(-(k*(a+b)), a+b, that) (oracle/ref_orbsites.cpp)
        const float t = a.fp_contract
                            ? __fmaf_rn(-__fmul_rn(kHarrisK, s2), s2, __fmaf_rn(fa, fb, -__fmul_rn(fc, fc)))
                            : __fsub_rn(__fsub_rn(__fmul_rn(fa, fb), __fmul_rn(fc, fc)),
                                        __fmul_rn(__fmul_rn(kHarrisK, s2), s2));
        const float resp = __fmul_rn(t, kHarrisScale4);
        dst[i] = (uint64_t)harris_key(resp) << 32 | (e & 0xFFFFFFu);
    }
}

// E = uint32_t (FAST score entries) or uint64_t (Harris-keyed entries)
template <typename E>
__device__ inline E* cell_entries(const ExtractArgs& a)
{
    if constexpr (sizeof(E) == 8) return a.cell_keys64;
    else return a.cell_lists;
}
template <typename E>
__device__ inline E* level_entries(const ExtractArgs& a)
{
    if constexpr (sizeof(E) == 8) return a.level_keys64;
    else return a.level_keys;
}

template <typename E>
__global__ __launch_bounds__(256) void k_retain_cells(ExtractArgs a, int waves_per_block, int wave_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sbuf[];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int cell = blockIdx.x * waves_per_block + wv, f = blockIdx.y;
    if (cell >= a.ncells) return;
    E* list = reinterpret_cast<E*>(sbuf + (size_t)wv * wave_words);
    int* pos = reinterpret_cast<int*>(list + kRetainCellCap);
    const CellGeom C = cget(a.cells, cell);
    const LevelGeom L = cget(a.levels, C.level);
    const int c = cell - L.cell_base;
    const int32_t* counts = a.cell_count + (size_t)f * a.ncells + L.cell_base;
    int k, pre, level_total;
    level_quota(a, L, counts, c, &k, &pre, &level_total);
    if (c == 0 && lane == 0) a.level_count[(size_t)f * a.nlevels + C.level] = min(level_total, L.level_cap);
    if (level_total > L.level_cap) {
        if (lane == 0) atomicOr(a.error_flags, 2);
        return;
    }
    const int n = counts[c];
    if (n == 0 || k == 0) return;
    const int take = min(n, k);
    E* src = cell_entries<E>(a) + (size_t)f * a.list_entries + C.list_off;
    E* dst = level_entries<E>(a) + (size_t)f * a.level_entries + L.level_off + pre;
    if (n > k && n <= 64) {
        // one entry per lane from the start: no staging
        const E v = wave_nth_element_small(lane < n ? src[lane] : E(0), n, k, list, a.nth_pivot);
        if (lane < take) dst[lane] = v;
    } else if (n > k && n <= kRetainCellCap) {
        stage_to_lds<8>(list, n, lane, 64, [&](int i) { return src[i]; });
        lds_wave_sync();
        wave_nth_element(list, n, k, pos, a.nth_pivot);
        for (int i = lane; i < take; i += 64) dst[i] = list[i];
    } else if (n > k) {
        // long list: replay in place in global memory
        int* gpos = a.retain_scratch + (size_t)f * (a.list_entries + 4 * a.ncells) + C.list_off + 4 * cell;
        wave_nth_element<true>(src, n, k, gpos, a.nth_pivot);
        for (int i = lane; i < take; i += 64) dst[i] = src[i];
    } else {
        for (int i = lane; i < take; i += 64) dst[i] = src[i];
    }
}

template <typename E>
__global__ __launch_bounds__(256) void k_retain_levels(ExtractArgs a, int waves_per_block, int wave_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sbuf[];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int level = blockIdx.x * waves_per_block + wv, f = blockIdx.y;
    if (level >= a.nlevels) return;
    const LevelGeom L = cget(a.levels, level);
    int32_t* cnt = a.level_count + (size_t)f * a.nlevels + level;
    const int nlev = *cnt;
    if (nlev <= L.n_desired) return;
    E* list = reinterpret_cast<E*>(sbuf + (size_t)wv * wave_words);
    int* pos = reinterpret_cast<int*>(list + a.max_level_cap);
    E* g = level_entries<E>(a) + (size_t)f * a.level_entries + L.level_off;
    stage_to_lds<8>(list, nlev, lane, 64, [&](int i) { return g[i]; });
    lds_wave_sync();
    wave_nth_element(list, nlev, L.n_desired, pos, a.nth_pivot);
    for (int i = lane; i < L.n_desired; i += 64) g[i] = list[i];
    if (lane == 0) *cnt = L.n_desired;
}

// ---------------------------------------------------------------------------
// GaussianBlur 7x7, sigma 2, BORDER_REFLECT_101 on the level ROI with the
// parent border as context (OpenCV 2.4 8U fixed-point separable filter:
// taps {18,34,49,55,49,34,18}/256 per pass).  Column pass rounding: columns
// < nvec follow SymmColumnVec_32s8u (float, round-half-even), the tail
// FixedPtCastEx (+2^15 >> 16).  The padded border is copied unblurred.
// Each thread owns one dword column (4 pixels) of a kBlurStrip-row strip and
// slides a 7-row window of horizontal sums down it in registers: one pass
// over the input rows it needs, one dword store per output row, no LDS.
// ---------------------------------------------------------------------------
typedef float orbx_f2 __attribute__((ext_vector_type(2)));

// Horizontal pass of one dword (4 pixels; wl / wr: its left / right
// neighbours): the four row sums as two packed float pairs.
// bias: blur_bias().  The sums arrive as the floats 2^23 + h; one packed
// subtraction of 2^23 per pair (exact) leaves the floats (float)h.
__device__ __forceinline__ void blur_hrow(uint32_t wl, uint32_t wc, uint32_t wr, uint32_t bias, orbx_f2 (&o)[2])
{
    uint32_t hs[4];
    blur_hsum_w(wl, wc, wr, bias, hs);
    const orbx_f2 kOff = {8388608.0f, 8388608.0f};
    o[0] = orbx_f2{__uint_as_float(hs[0]), __uint_as_float(hs[1])} - kOff;
    o[1] = orbx_f2{__uint_as_float(hs[2]), __uint_as_float(hs[3])} - kOff;
}

// Vertical pass of one dword over the 7 rows of horizontal sums R, in packed
// FP32 (two pixels per v_pk_fma_f32): the row sums are integers <= 255 * 257
// and N <= 255 * 257^2; every partial sum below 2^24 is exact, and an N beyond
// 2^24 saturates to 255 either way.  Rounding and saturation by
// v_cvt_pk_u8_f32 (round half to even = cvtps2dq of SymmColumnVec_32s8u); the
// scalar tail columns (FixedPtCastEx, +2^15 >> 16) pass
// floor((N + 2^15) / 2^16).  The taps carry the 1/65536: a power of two, so
// every product and partial sum is the integer form's times 2^-16, still
// exact.  Bytes that are not `inside` keep `raw`'s.
__device__ __forceinline__ uint32_t blur_vstep(const orbx_f2 (&R)[7][2], uint32_t raw, const bool (&inside)[4],
                                               const bool (&tail_col)[4], bool any_tail)
{
    constexpr float kInv = 1.0f / 65536.0f;
    constexpr float k0 = 55.0f * kInv, k1 = 49.0f * kInv, k2 = 34.0f * kInv, k3 = 18.0f * kInv;
    float sv[4];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        orbx_f2 N = R[3][h] * k0;
        N = __builtin_elementwise_fma(R[2][h] + R[4][h], orbx_f2{k1, k1}, N);
        N = __builtin_elementwise_fma(R[1][h] + R[5][h], orbx_f2{k2, k2}, N);
        N = __builtin_elementwise_fma(R[0][h] + R[6][h], orbx_f2{k3, k3}, N);
        sv[2 * h] = N.x;
        sv[2 * h + 1] = N.y;
        if (any_tail) {
            const orbx_f2 tl2 = N + 0.5f;
            if (tail_col[2 * h]) sv[2 * h] = floorf(tl2.x);
            if (tail_col[2 * h + 1]) sv[2 * h + 1] = floorf(tl2.y);
        }
    }
    uint32_t word = raw;   // border columns keep the raw byte
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (inside[j]) word = __builtin_amdgcn_cvt_pk_u8_f32(sv[j], j, word);
    return word;
}

// One blur work block (bx) of frame f.
__device__ __forceinline__ void blur_block(const ExtractArgs& a, const int4* tiles, const int bx, const int f)
{
    // One wave per (row strip, chunk of kBlurChunkCols dword columns): lane
    // l holds dword 62 c - 1 + l of each row, lanes 0 and 63 only as halo.
    // A row is one dword load per lane; the left / right neighbour dwords of
    // the horizontal taps come from the adjacent lanes (DPP wave_shr:1 /
    // wave_shl:1) instead of two more loads.
    const int4 tl = cget(tiles, bx);   // level, first wave item, chunks per row, strips
    const int wi = tl.y + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wi >= tl.z * tl.w) return;       // whole waves
    const LevelGeom L = cget(a.levels, tl.x);
    const int strip = wi / tl.z, chunk = wi - strip * tl.z;
    const int ndw = L.stride >> 2;
    const int dw = kBlurChunkCols * chunk - 1 + lane;
    const bool out = lane >= 1 && lane <= kBlurChunkCols && dw < ndw;
    const int x = 4 * min(max(dw, 0), ndw - 1);
    const int y0 = strip * kBlurStrip, y1 = min(y0 + kBlurStrip, L.ph);
    // uniform level bases + 32-bit per-lane offsets (saddr + voffset loads)
    const uint8_t* src = a.pyr_raw + (size_t)f * a.frame_pyr_bytes + L.off;
    uint8_t* dst = a.pyr_blur + (size_t)f * a.frame_pyr_bytes + L.off;
    const uint32_t stride = (uint32_t)L.stride;
    auto ld = [&](int y) { return *reinterpret_cast<const uint32_t*>(src + ((uint32_t)y * stride + (uint32_t)x)); };
    auto st = [&](int y, uint32_t v) {
        if (out) *reinterpret_cast<uint32_t*>(dst + ((uint32_t)y * stride + (uint32_t)x)) = v;
    };
    // neighbours' words (lane - 1 / lane + 1): the DPP reads need every lane
    // of the wave active, so all lanes run the same rows
    auto left = [&](uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false); };
    auto right = [&](uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, false); };
    // interior rows of this level in padded coordinates: rows [ya, yb) of the
    // strip are blurred (border columns keep their raw bytes), the rest copied
    const int iy0 = kEdge, iy1 = kEdge + L.h;
    const int ya = min(max(y0, iy0), y1), yb = max(min(y1, iy1), ya);
    // bytes beyond the padded width (row pitch padding) are zero
    uint32_t keep_mask = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (x + j < L.pw) keep_mask |= 0xFFu << (8 * j);
    // copied (border) rows, 4 loads in flight per round
    auto copy_rows = [&](int ylo, int yhi) {
        for (int yc = ylo; yc < yhi; yc += 4) {
            uint32_t v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = ld(min(yc + k, yhi - 1));
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (yc + k < yhi) st(yc + k, v[k] & keep_mask);
        }
    };
    copy_rows(y0, ya);
    if (ya < yb) {
        // per column: float path (round half to even) below nvec, else +2^15
        int half_even[4];
        bool inside[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int xi = x + j - kEdge;
            inside[j] = xi >= 0 && xi < L.w;
            half_even[j] = xi < L.nvec_blur;
        }
        bool tail_col[4], any_tail = false;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            tail_col[j] = inside[j] && !half_even[j];
            any_tail = any_tail || tail_col[j];
        }
        orbx_f2 R[7][2];
        const uint32_t bias = blur_bias();
        auto hrow = [&](uint32_t c, orbx_f2 (&o)[2]) { blur_hrow(left(c), c, right(c), bias, o); };
        uint32_t C[3];   // raw centre words of rows y, y+1, y+2 (loaded as rows y'+3 earlier)
        {
            uint32_t w0[6];
#pragma unroll
            for (int k = 0; k < 6; k++) w0[k] = ld(ya - 3 + k);
#pragma unroll
            for (int k = 0; k < 6; k++) {
                hrow(w0[k], R[k]);
                if (k >= 3) C[k - 3] = w0[k];
            }
        }
        // chunks of 7 output rows (the window's period: the register
        // rotation needs no moves); the chunk's input rows y + 3 are loaded
        // together, then filtered from registers
        constexpr int kBlurChunk = 7;
        for (int yc = ya; yc < yb; yc += kBlurChunk) {
            uint32_t wc[kBlurChunk];
#pragma unroll
            for (int k = 0; k < kBlurChunk; k++) wc[k] = ld(min(yc + k, yb - 1) + 3);   // rows past yb + 2 repeat
#pragma unroll
            for (int k = 0; k < kBlurChunk; k++) {
                // rows past yb are computed on repeated input and not stored:
                // no early exit, so the window rotation stays straight-line
                const int y = yc + k;
                hrow(wc[k], R[6]);
                const uint32_t word = blur_vstep(R, C[0], inside, tail_col, any_tail);
                if (y < yb) st(y, word & keep_mask);
#pragma unroll
                for (int kk = 0; kk < 6; kk++)
#pragma unroll
                    for (int h = 0; h < 2; h++) R[kk][h] = R[kk + 1][h];
                C[0] = C[1];
                C[1] = C[2];
                C[2] = wc[k];
            }
        }
    }
    copy_rows(yb, y1);
}

__global__ __launch_bounds__(256) void k_blur(ExtractArgs a, const int4* tiles)
{
    blur_block(a, tiles, (int)blockIdx.x, (int)blockIdx.y);
}

// ---------------------------------------------------------------------------
// IC_Angle + computeOrbDescriptor + output assembly, one wave per keypoint.
// The wave first stages, with independent dword loads, one unblurred window
// per keypoint in LDS: rows Y - 21 .. Y + 21, 12 dwords per row from
// (X - 21) & ~3.  It holds the 31x31 patch of IC_Angle (radius 15) and every
// tap of the 37x37 blurred patch of the descriptor (rotated pattern points
// reach cvRound(13*sqrt(2)) = 18, the 7x7 filter 3 more).  Keypoints lie in
// [16, w - 16) x [16, h - 16) of the level and the padded border is 16, so
// the window stays inside the padded level; a window that leaves the level's
// interior is staged from its REFLECT_101 sources inside the level
// (describe_stage_reflect), so no border byte is ever read.  After IC_Angle
// the half-wave blurs the 37x37 patch in place (describe_blur_window): the
// whole-level blur pass and its second pyramid are not on the extraction path.
// ---------------------------------------------------------------------------
constexpr int kIcRows = 2 * kHalfPatch + 1;          // 31
constexpr int kBrR = 18;                             // pattern reach
constexpr int kBrRows = 2 * kBrR + 1;                // 37
constexpr int kWinR = kBrR + 3;                      // + the filter's reach
constexpr int kWinRows = 2 * kWinR + 1;              // 43
constexpr int kWinDw = 12;                           // dwords per window row
constexpr int kBrPitch = 4 * kWinDw;                 // 48: window row pitch (raw and blurred)
constexpr int kWinPad = 16;                          // in front: dword column 0's left neighbour reads into it
constexpr int kDescWaveBytes = kWinPad + kWinRows * kBrPitch;   // 2080 per keypoint
constexpr int kWinCols = 10;                         // dword columns that hold the 37 blurred bytes
constexpr int kWinStrips = 3;                        // row strips per column; 30 of the 32 lanes work
constexpr int kWinStripRows = 13;                    // rows 0..12, 12..24, 24..36 (rows 12 and 24 twice)
static_assert(kWinCols * kWinStrips <= 32 && (kWinStrips - 1) * (kWinStripRows - 1) + kWinStripRows == kBrRows,
              "the strips of one half-wave cover the blurred patch");

// Orders a half-wave's LDS writes before the other lanes' reads (and the
// reverse): one wave, so no hardware barrier.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The window of a keypoint near the level's edge.  No border is read: the
// batch resize writes level interiors only, and the direct level 0 is the
// frame itself (level_src), where none exists.  The window's first byte is
// padded position (x0, y0); every byte is fetched from the interior position
// BORDER_REFLECT_101 maps it to, so the staged bytes equal the padded level's
// and every address lies inside the level's interior (the frame, for the
// direct level 0) -- also for the window bytes that the blur never uses.
// Keypoints are at least kEdge inside the level, so the window lies within
// the padded level's kEdge border and one reflection per index is enough (the
// clamps only keep a degenerate tiny level in bounds).
// x0 and kEdge are multiples of 4, so a window dword at level columns
// c .. c + 3 lies wholly left of the level (c <= -4) or starts inside it or
// behind it.  A lane owns one dword column of the window and every second
// row (lane hl: column hl & 15 of the kWinDw, rows (hl >> 4) + 2 t), so what
// depends on the column is computed once per lane: the source column of its
// one (unaligned) dword load d per row, and the byte selector that turns d
// into the window dword --
//   c < 0            d = columns -c - 3 .. -c, byte-reversed;
//   c >= lw          d = columns 2 lw - 5 - c .. 2 lw - 2 - c, byte-reversed;
//   c <= lw - 4      d = columns c .. c + 3, as loaded;
//   else (n = lw - c of 1 .. 3 bytes inside; widths that are no multiple of
//   4): d = columns lw - 4 .. lw - 1.  Byte j < n is column c + j, d's byte
//   4 - n + j; byte j >= n reflects to column lw - 2 + n - j, d's byte
//   2 + n - j (n = 1: the reversal again).
// Per row only the reflected row index and the address remain.  No branch
// per item, all of a lane's loads in flight together as in the common path;
// lanes 12 .. 15 of each 16 repeat column 11 and the odd rows' last item
// repeats row kWinRows - 1 (the same values to the same addresses).
__device__ __forceinline__ void describe_stage_reflect(const uint8_t* lev, int stride, int lw, int lh, int x0, int y0,
                                                       uint32_t* w32, int hl)
{
    constexpr int nld = (kWinRows + 1) / 2;
    static_assert(kWinDw <= 16, "a row's dword columns fit 16 lanes");
    const uint8_t* img = lev + (long long)kEdge * stride + kEdge;   // the level's first interior pixel
    const int j = min(hl & 15, kWinDw - 1), ph = hl >> 4;
    const int c = x0 - kEdge + 4 * j, nin = lw - c;   // nin: bytes of the dword inside the level, where 1 .. 3
    int col = c < 0 ? -c - 3 : (nin <= 0 ? 2 * lw - 5 - c : c);
    col = min(max(col, 0), lw - 4);
    const uint32_t sel = (c < 0 || nin <= 1) ? 0x00010203u : (nin == 2 ? 0x01020302u : (nin == 3 ? 0x02030201u : 0x03020100u));
    const uint8_t* src = img + col;
    const int ytop = y0 - kEdge + ph, ymir = 2 * lh - 2;
    uint32_t v[nld];
#pragma unroll
    for (int t = 0; t < nld; t++) {
        int y = ytop + (t < nld - 1 ? 2 * t : kWinRows - 1 - ph);
        y = max(y, -y);
        y = min(y, ymir - y);
        y = min(max(y, 0), lh - 1);
        uint32_t d;
        __builtin_memcpy(&d, src + (uint32_t)(y * stride), 4);
        v[t] = __builtin_amdgcn_perm(0u, d, sel);
    }
    uint32_t* dst = w32 + ph * kWinDw + j;
#pragma unroll
    for (int t = 0; t < nld; t++) dst[(t < nld - 1 ? 2 * t : kWinRows - 1 - ph) * kWinDw] = v[t];
}

// Stages the raw window of the keypoint at padded level position (X, Y) into
// win (kWinRows * kBrPitch bytes behind the keypoint's kWinPad), lane hl of
// 32; lev: the padded level's origin (for the direct level 0 the frame's
// virtual padded origin, level_src), lw x lh the level's size.  The loads
// below apply when the whole window (kWinRows rows x kBrPitch bytes) lies
// inside the level's interior; other windows go through
// describe_stage_reflect -- one rule for every level and mode, whether or not
// a border was ever written.  A row is kWinPieces 16-byte pieces and win's
// rows are contiguous, so piece p (row p / 3) goes to win + 16 p: lane hl
// takes pieces hl, hl + 32, ... with 16-byte loads (the window origin is
// 4-byte aligned only) and 16-byte LDS stores at a constant distance; the one
// piece left over after kStageRounds rounds is loaded by every lane and
// stored by lane 0.  All loads in flight together; 32-bit offsets from the
// window's first row.  Returns the window centre's byte offset in win.
typedef uint32_t stage_piece_t __attribute__((ext_vector_type(4), aligned(4)));
constexpr int kWinPieces = kBrPitch / 16;            // 3 per row
constexpr int kStagePieces = kWinRows * kWinPieces;   // 129
constexpr int kStageRounds = kStagePieces / 32;       // 4 full rounds of 32 lanes
static_assert(kBrPitch % 16 == 0 && kWinPad % 16 == 0 && kDescWaveBytes % 16 == 0,
              "every 16-byte piece of a window is 16-byte aligned in LDS");
static_assert(kStagePieces - 32 * kStageRounds == 1, "one piece is left over after the full rounds");
static_assert(kStagePieces < 512, "p / 3 == p * 171 >> 9 holds below 512");
__device__ __forceinline__ int describe_stage_window(const uint8_t* lev, uint32_t stride, int lw, int lh, int X, int Y,
                                                     uint8_t* win, int hl)
{
    const int x0 = (X - kWinR) & ~3;
    if (Y - kWinR < kEdge || Y + kWinR >= kEdge + lh || x0 < kEdge || x0 + kBrPitch > kEdge + lw) {
        describe_stage_reflect(lev, (int)stride, lw, lh, x0, Y - kWinR, reinterpret_cast<uint32_t*>(win), hl);
        return kWinR * kBrPitch + (X - x0);
    }
    const uint8_t* r0 = lev + (long long)(Y - kWinR) * stride + x0;
    // piece p at row r = p / 3 lies at r * stride + 16 (p - 3 r) = r * (stride - kBrPitch) + 16 p
    const uint32_t skip = stride - kBrPitch;
    stage_piece_t v[kStageRounds + 1];
#pragma unroll
    for (int k = 0; k < kStageRounds; k++) {
        const uint32_t p = (uint32_t)hl + 32u * k, r = (p * 171u) >> 9;
        v[k] = *reinterpret_cast<const stage_piece_t*>(r0 + (__umul24(r, skip) + 16u * p));   // strides are < 2^24
    }
    v[kStageRounds] = *reinterpret_cast<const stage_piece_t*>(
        r0 + ((uint32_t)(kWinRows - 1) * stride + 16u * (kWinPieces - 1)));
    uint4* w128 = reinterpret_cast<uint4*>(win);
#pragma unroll
    for (int k = 0; k < kStageRounds; k++) w128[hl + 32 * k] = uint4{v[k].x, v[k].y, v[k].z, v[k].w};
    if (hl == 0)
        w128[kStagePieces - 1] =
            uint4{v[kStageRounds].x, v[kStageRounds].y, v[kStageRounds].z, v[kStageRounds].w};
    return kWinR * kBrPitch + (X - x0);
}

// GaussianBlur 7x7 of the 37x37 patch around (X, Y) inside the staged raw
// window, in place: k_blur's filter (blur_hrow, blur_vstep) and its rules per
// byte at level position (xi, yi): outside [0, w) x [0, h) the raw border
// byte, inside the 7x7 result over the raw padded pixels, with the float
// rounding for xi < nvec and the tail rounding beyond.  Lane hl owns one
// dword column and one strip of kWinStripRows rows; it slides a 7-row window
// of horizontal sums down the strip in registers and keeps its output words
// there until every lane has read its raw rows.  Bytes of the 10 dword
// columns outside the 37x37 patch are undefined.
__device__ __forceinline__ void describe_blur_window(uint8_t* win, int X, int Y, int lw, int lh, int nvec, int hl)
{
    const int x0 = (X - kWinR) & ~3;
    const int d0 = (X - x0 - kBrR) >> 2;   // first dword column with patch bytes: 0 or 1
    const bool act = hl < kWinCols * kWinStrips;
    const int strip = min(hl / kWinCols, kWinStrips - 1), d = d0 + (hl - (hl / kWinCols) * kWinCols);
    const int j0 = strip * (kWinStripRows - 1);   // first patch row of the strip = its first input row of the window
    // dword column 0 has no left neighbour (the read falls into the previous
    // row or kWinPad): only its byte 3 can be a patch byte (d0 = 0: the patch
    // starts at byte 3), and that sum does not read the left word
    uint32_t* wp = reinterpret_cast<uint32_t*>(win) + j0 * kWinDw + d;
    const bool all[4] = {true, true, true, true};
    bool tail_col[4], any_tail = false;
    uint32_t in_mask = 0;   // bytes inside the level's columns
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int xi = x0 + 4 * d + j - kEdge;
        const bool inside = xi >= 0 && xi < lw;
        if (inside) in_mask |= 0xFFu << (8 * j);
        tail_col[j] = inside && xi >= nvec;
        any_tail = any_tail || tail_col[j];
    }
    const int yi0 = Y - kBrR + j0 - kEdge;   // level row of the strip's first output row
    uint32_t outw[kWinStripRows];
    const uint32_t bias = blur_bias();
    // tail: some lane of the wave has a tail column (rare: a keypoint within
    // 18 columns of the right edge of a level whose width is not vectorised
    // to the end); the common instance carries no tail arithmetic
    auto strip_rows = [&](auto tail) {
        orbx_f2 R[7][2];
        uint32_t C[3];   // raw centre words of the next three output rows
        uint32_t w[3];   // the next input row's left, centre and right words
        auto ldrow = [&](int r) {
#pragma unroll
            for (int i = 0; i < 3; i++) w[i] = wp[r * kWinDw - 1 + i];
        };
        // one row's words are read ahead of the row being filtered, no more
        // (the scheduler would otherwise hoist every read and spill)
        auto hrow = [&](int r, orbx_f2 (&o)[2]) {
            const uint32_t l = w[0], c = w[1], rr = w[2];
            if (r + 1 <= kWinStripRows + 5) ldrow(r + 1);
            blur_hrow(l, c, rr, bias, o);
            __builtin_amdgcn_sched_barrier(0);
            return c;
        };
        ldrow(0);
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const uint32_t c = hrow(k, R[k]);
            if (k >= 3) C[k - 3] = c;
        }
#pragma unroll
        for (int k = 0; k < kWinStripRows; k++) {
            const uint32_t c = hrow(k + 6, R[6]);
            // border rows and columns keep the raw bytes
            const uint32_t word = blur_vstep(R, 0u, all, tail_col, decltype(tail)::value);
            const uint32_t m = (unsigned)(yi0 + k) < (unsigned)lh ? in_mask : 0u;
            outw[k] = (word & m) | (C[0] & ~m);
#pragma unroll
            for (int kk = 0; kk < 6; kk++)
#pragma unroll
                for (int h = 0; h < 2; h++) R[kk][h] = R[kk + 1][h];
            C[0] = C[1];
            C[1] = C[2];
            C[2] = c;
        }
    };
    if (__any(any_tail)) strip_rows(std::true_type{});
    else strip_rows(std::false_type{});
    wave_lds_sync();
    if (act) {
#pragma unroll
        for (int k = 0; k < kWinStripRows; k++) wp[(k + 3) * kWinDw] = outw[k];
    }
    wave_lds_sync();
}

// Half-wave (32-lane) sums: DPP row shifts inside each 16-lane row, then
// row_bcast:15 folds row 0 into row 1 and row 2 into row 3; lane 31 holds the
// lower half's sum, lane 63 the upper half's.
__device__ inline int half_wave_sum(int v)
{
    v += dpp_or0<0x111, 0xf>(v);
    v += dpp_or0<0x112, 0xf>(v);
    v += dpp_or0<0x114, 0xf>(v);
    v += dpp_or0<0x118, 0xf>(v);
    v += dpp_or0<0x142, 0xa>(v);
    const int lo = __builtin_amdgcn_readlane(v, 31), hi = __builtin_amdgcn_readlane(v, 63);
    return (threadIdx.x & 32) ? hi : lo;
}

// IC_Angle (src/ORBextractor.cc:124-151) on the staged raw window, by rows:
// lane hl of the half owns row v = hl - 15 of the circular patch (lane 31:
// the table's row of zeros).  The moments are integer sums, exact in any
// order: m01 = sum_v v * S1(v) and m10 = sum_v (Su(v) - 16 S1(v)) with
// S1 = sum_u inside * I and Su = sum_u (u + 16) * inside * I over the row's
// bytes u = -15 .. 16.  Those 32 bytes start at window byte (X - x0) - 15 =
// 6 .. 9 of the row: nine aligned dwords, shifted into place by a byte count
// that is uniform in the half, then one v_dot4_u32_u8 per dword and sum
// against the row's weights (ic_row_table: 0 outside the circle, which also
// drops the byte at u = 16).  Every partial stays below 2^23.
// describe_ic_weights: the lane's table row, loaded ahead of the staging.
__device__ __forceinline__ void describe_ic_weights(const uint32_t* ic_rows, int hl, uint32_t (&t)[kIcTabDw])
{
    const int row = min(abs(hl - kHalfPatch), kHalfPatch + 1);
    const uint4* p = reinterpret_cast<const uint4*>(ic_rows + row * kIcTabDw);
#pragma unroll
    for (int q = 0; q < kIcTabDw / 4; q++) {
        const uint4 w = p[q];
        t[4 * q] = w.x;
        t[4 * q + 1] = w.y;
        t[4 * q + 2] = w.z;
        t[4 * q + 3] = w.w;
    }
}

// win: the staged window of the keypoint at padded level column X; returns
// the half's moments in every lane of the half.
__device__ __forceinline__ void describe_moments(const uint8_t* win, int X, int hl, const uint32_t (&t)[kIcTabDw],
                                                 int& m01, int& m10)
{
    static_assert(kIcTabDw == 16 && ((kWinR - kHalfPatch + 3) & ~3) + 36 <= kBrPitch &&
                      kWinR - kHalfPatch + kIcRows < kWinRows,
                  "nine dwords from the row's byte 4 or 8 stay inside the row, lane 31's row inside the window");
    const int b0 = kWinR - kHalfPatch + ((X - kWinR) & 3);   // the row's byte of u = -15
    const uint32_t* row = reinterpret_cast<const uint32_t*>(win) + (kWinR - kHalfPatch + hl) * kWinDw + (b0 >> 2);
    uint32_t w[9];
#pragma unroll
    for (int i = 0; i < 9; i++) w[i] = row[i];
    const uint32_t sh = (uint32_t)b0 & 3u;
    uint32_t s1 = 0, su = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t d = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
        s1 = __builtin_amdgcn_udot4(d, t[i], s1, false);
        su = __builtin_amdgcn_udot4(d, t[8 + i], su, false);
    }
    m01 = half_wave_sum((hl - kHalfPatch) * (int)s1);
    m10 = half_wave_sum((int)su - 16 * (int)s1);
}

// Two keypoints per wave, one per 32-lane half, eight per workgroup: the
// per-keypoint scalar steps (fastAtan2, the correctly rounded sin/cos) run
// once per workgroup, one keypoint per lane of one wave, and the pattern's
// 256 tests map onto 8 rounds of 32 lanes (ballot halves = 32 descriptor
// bits each).
// GET_VALUE's sample coordinates (src/ORBextractor.cc:165-167): row
// x*b + y*a and column x*a - y*b.  kFma: as GCC contracts them on an FMA host
// (-O3 -march=native, CMakeLists.txt:12-13): fma(x, b, y*a), fma(x, a, -(y*b)).
template <bool kFma>
__device__ inline int orb_sample_offset(float px, float py, float sa, float ca)
{
    const float fy = kFma ? __fmaf_rn(px, sa, __fmul_rn(py, ca)) : __fadd_rn(__fmul_rn(px, sa), __fmul_rn(py, ca));
    const float fx = kFma ? __fmaf_rn(px, ca, -__fmul_rn(py, sa)) : __fsub_rn(__fmul_rn(px, ca), __fmul_rn(py, sa));
    return cv_round(fy) * kBrPitch + cv_round(fx);
}

// Both points of a pattern pair at once on packed fp32 (v_pk_mul_f32 /
// v_pk_add_f32 / v_pk_fma_f32: each lane rounds exactly as the scalar
// operation).  cvRound (round half to even, OpenCV 2.4's cvtsd2si) is the
// 1.5 * 2^23 magic-number round trip: |coordinate| <= 18, so fy + M rounds fy
// to its nearest-even integer and subtracting M again is exact.  The patch
// offset row * kBrPitch + col (+ base, folded into the column's round trip)
// is then an exact float fma on integers below 2^24.  Returns the two LDS
// byte addresses.
template <bool kFma>
__device__ inline void orb_sample_addr2(orbx_f2 px, orbx_f2 py, float sa, float ca, float base, uint32_t& a1,
                                        uint32_t& a2)
{
    const orbx_f2 SA = {sa, sa}, CA = {ca, ca};
    orbx_f2 fy, fx;
    if constexpr (kFma) {
        fy = __builtin_elementwise_fma(px, SA, py * CA);
        fx = __builtin_elementwise_fma(px, CA, -(py * SA));
    } else {
        fy = px * SA + py * CA;
        fx = px * CA - py * SA;
    }
    const orbx_f2 M = {12582912.0f, 12582912.0f}, MB = {12582912.0f - base, 12582912.0f - base};
    const orbx_f2 P = {(float)kBrPitch, (float)kBrPitch};
    const orbx_f2 ry = (fy + M) - M, rxb = (fx + M) - MB;
    const orbx_f2 ad = __builtin_elementwise_fma(ry, P, rxb);
    a1 = (uint32_t)ad.x;
    a2 = (uint32_t)ad.y;
}

// fastAtan2's angle and its correctly rounded sin / cos, one per keypoint
struct DescTrig {
    float angle, sa, ca;
};

// 5 waves per SIMD: the register allocator otherwise spends past 128 VGPRs
// on hoisted window reads (the kernel is VALU-bound; 90 VGPRs, no spills)
template <bool kFma>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void k_describe(ExtractArgs a, int nframes)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_patch[2 * kWaves][kDescWaveBytes];
    __shared__ int2 s_mom[2 * kWaves];       // m01, m10 per keypoint of the workgroup
    __shared__ DescTrig s_trig[2 * kWaves];
    // XCD-aware order (xcd_block): a frame's keypoint patches, which overlap,
    // are fetched into one XCD's L2
    const XcdBlock xb = xcd_block();
    const int f = xb.frame, chunk = xb.chunk;
    if (f >= nframes) return;
    // wv is wave-uniform: with it in a scalar register the search for the two
    // keypoints' levels below runs on the scalar unit
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & (kWaves - 1);
    const int half = lane >> 5, hl = lane & 31;
    const int slot = wv * 2 + half;
    const int k0 = chunk * (2 * kWaves) + wv * 2, k = k0 + half;
    // tables needed later, loaded up front (independent of the keypoint):
    // this lane's row of IC_Angle's weights, its 8 pattern pairs
    uint32_t icw[kIcTabDw];
    describe_ic_weights(a.ic_rows, hl, icw);
    uint32_t pat[8];
#pragma unroll
    for (int r = 0; r < 8; r++) pat[r] = *reinterpret_cast<const uint32_t*>(c_pattern[r * 32 + hl]);
    // per-level data, one level per lane, fetched in the same round trip as
    // the tables above: keypoint count, offsets, stride, scale, patch size
    const int ll = min(lane, a.nlevels - 1);
    const int cnt_l = lane < a.nlevels ? a.level_count[(size_t)f * a.nlevels + lane] : 0;
    const long long off_l = a.levels[ll].off;
    const int stride_l = a.levels[ll].stride, loff_l = a.levels[ll].level_off;
    const int w_l = a.levels[ll].w, h_l = a.levels[ll].h, nvec_l = a.levels[ll].nvec_blur;
    const float scale_l = a.levels[ll].scale, psize_l = a.levels[ll].patch_size;
    // keypoints k0 (lower half) and k0 + 1 (upper half): level and index in it
    int total = 0, level0 = -1, local0 = 0, level1 = -1, local1 = 0;
    for (int l = 0; l < a.nlevels; l++) {
        const int c = __builtin_amdgcn_readlane(cnt_l, l);
        if (level0 < 0 && k0 < total + c) {
            level0 = l;
            local0 = k0 - total;
        }
        if (level1 < 0 && k0 + 1 < total + c) {
            level1 = l;
            local1 = k0 + 1 - total;
        }
        total += c;
    }
    int level = half ? level1 : level0, local = half ? local1 : local0;
    if (k == 0 && lane == 0) {
        a.out_n[a.first_slot + f] = total;
        if (a.host_out) {   // every earlier kernel's error flags are final here
            reinterpret_cast<int32_t*>(a.host_out)[0] = total;
            reinterpret_cast<int32_t*>(a.host_out)[1] = *a.error_flags;
        }
    }
    // no keypoint in the whole workgroup (block-uniform: every wave computes
    // the same total): nothing to do, and no barrier is reached
    if (chunk * (2 * kWaves) >= total) return;
    // a wave works while either half has a keypoint (DPP/ballot need the
    // whole wave); an empty half works on level 0 / key 0 and stores nothing.
    // A wave without a keypoint only takes part in the block barriers.
    const bool valid = level >= 0;
    const bool wave_on = level0 >= 0;   // k0 + 1 has a keypoint only if k0 has
    if (!valid) {
        level = 0;
        local = 0;
    }
    int x = 0, y = 0, X = 0, Y = 0, lev_w = 0, lev_h = 0, lev_nvec = 0;
    float lev_scale = 0.f, lev_psize = 0.f, response = 0.f;
    uint8_t* win = s_patch[slot] + kWinPad;
    const uint8_t* br = win;
    int m01 = 0, m10 = 0;
    if (wave_on) {
        // this half's level data, read back from lane `level` (one
        // ds_bpermute_b32 per value, no LDS memory involved)
        auto pick = [&](int v) { return __builtin_amdgcn_ds_bpermute(level << 2, v); };
        const long long lev_off = (long long)(((unsigned long long)(uint32_t)pick((int)(off_l >> 32)) << 32) |
                                              (uint32_t)pick((int)off_l));
        const int lev_stride = pick(stride_l), lev_loff = pick(loff_l);
        lev_w = pick(w_l);
        lev_h = pick(h_l);
        lev_nvec = pick(nvec_l);
        lev_scale = __int_as_float(pick(__float_as_int(scale_l)));
        lev_psize = __int_as_float(pick(__float_as_int(psize_l)));
        uint32_t e;
        if (a.harris) {
            const uint64_t e64 = a.level_keys64[(size_t)f * a.level_entries + lev_loff + local];
            e = (uint32_t)e64;
            response = harris_response((uint32_t)(e64 >> 32));
        } else {
            e = a.level_keys[(size_t)f * a.level_entries + lev_loff + local];
            response = (float)(e >> 24);   // FAST score
        }
        y = (int)((e >> 12) & 0xFFF);
        x = (int)(e & 0xFFF);
        X = kEdge + (valid ? x : kHalfPatch + 8);
        Y = kEdge + (valid ? y : kHalfPatch + 8);
        // the raw window; br: its centre, the centre of the blurred patch
        // after describe_blur_window
        const LevelSrc ls = level_src(a, f, level, lev_off, lev_stride);
        br = win + describe_stage_window(ls.base, (uint32_t)ls.stride, lev_w, lev_h, X, Y, win, hl);
        wave_lds_sync();
        // IC_Angle on the unblurred level
        describe_moments(win, X, hl, icw, m01, m10);
    }
    // fastAtan2 and the correctly rounded sin/cos are one value per keypoint:
    // one wave of the workgroup (a different one from block to block, so the
    // work is spread over the SIMDs) computes them for all eight keypoints,
    // one per lane, between two block barriers.  The blur does not depend on
    // the angle and runs between the barriers too: the other waves blur while
    // the chosen wave does the trigonometry first.
    if (hl == 0) s_mom[slot] = int2{m01, m10};
    __syncthreads();
    if (wv == ((chunk + f) & (kWaves - 1)) && lane < 2 * kWaves) {
        const int2 m = s_mom[lane];
        const float ang = fast_atan2_deg((float)m.x, (float)m.y);
        const float factorPI = (float)(M_PI / 180.f);
        float s, c;
        cr_sincosf(__fmul_rn(ang, factorPI), &s, &c);
        s_trig[lane] = DescTrig{ang, s, c};
    }
    // the blurred patch overwrites the raw window, behind a wave_lds_sync
    // that follows every lane's IC_Angle reads
    if (wave_on) describe_blur_window(win, X, Y, lev_w, lev_h, lev_nvec, hl);
    __syncthreads();
    if (!wave_on) return;
    const float angle = s_trig[slot].angle, sa = s_trig[slot].sa, ca = s_trig[slot].ca;
    // computeOrbDescriptor on the blurred patch (src/ORBextractor.cc:155-194)
    uint8_t* desc = a.out_desc + ((size_t)(a.first_slot + f) * a.nfeatures + k) * 32;
    // the blurred patch centre as an offset into the block's LDS (exact in float)
    const uint8_t* lds_bytes = &s_patch[0][0];
    const float brf = (float)(int)(br - lds_bytes);
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const orbx_f2 px = {(float)(int8_t)(pat[r] & 0xFF), (float)(int8_t)((pat[r] >> 16) & 0xFF)};
        const orbx_f2 py = {(float)(int8_t)((pat[r] >> 8) & 0xFF), (float)(int8_t)(pat[r] >> 24)};
        uint32_t a1, a2;
        orb_sample_addr2<kFma>(px, py, sa, ca, brf, a1, a2);
        const int t0 = lds_bytes[a1];
        const int t1 = lds_bytes[a2];
        const unsigned long long bits = __ballot(t0 < t1);
        // this half's 32 bits are descriptor bits 32r .. 32r+31 (bytes 4r .. 4r+3)
        if (valid && hl == r) {
            reinterpret_cast<uint32_t*>(desc)[r] = (uint32_t)(bits >> (32 * half));
            if (a.host_out)
                reinterpret_cast<uint32_t*>(a.host_out + 64 + (size_t)a.nfeatures * sizeof(orbx_keypoint) +
                                            (size_t)k * 32)[r] = (uint32_t)(bits >> (32 * half));
        }
    }
    if (valid && hl == 0) {
        orbx_keypoint kp;
        kp.x = (float)x;
        kp.y = (float)y;
        if (level != 0) {
            kp.x = __fmul_rn(kp.x, lev_scale);
            kp.y = __fmul_rn(kp.y, lev_scale);
        }
        kp.size = lev_psize;
        kp.angle = angle;
        kp.response = response;
        kp.octave = level;
        kp.class_id = -1;
        a.out_kps[(size_t)(a.first_slot + f) * a.nfeatures + k] = kp;
        if (a.host_out) reinterpret_cast<orbx_keypoint*>(a.host_out + 64)[k] = kp;
    }
}

// Diagnostics: the LDS introselect replay of k_retain_cells on one list
// of u32 entries (key << 24 | payload) or u64 entries (key << 32 |
// payload), one wavefront; also the global-memory replay of long lists
// (out_glb).
template <typename E>
__global__ __launch_bounds__(64) void k_debug_nth(const E* in, int n, int nth, E* out_glb, E* out_lds, int* gpos,
                                                  int pivot_mode)
{
    __shared__ E list[kRetainCellCap];
    __shared__ int pos[kRetainCellCap + 8];
    const int lane = threadIdx.x;
    for (int i = lane; i < n; i += 64) out_glb[i] = in[i];
    global_wave_sync();
    wave_nth_element<true>(out_glb, n, nth, gpos, pivot_mode);
    for (int i = lane; i < n; i += 64) list[i] = in[i];
    lds_wave_sync();
    wave_nth_element(list, n, nth, pos, pivot_mode);
    for (int i = lane; i < n; i += 64) out_lds[i] = list[i];
}

// One list of n <= kRetainCellCap entries through both replays; host arrays.
template <typename E>
int debug_nth(const E* entries, int n, int nth, int pivot_mode, E* out_glb, E* out_lds)
{
    if (!entries || !out_glb || !out_lds || n < 0 || n > kRetainCellCap || nth < 0 || nth > n ||
        (pivot_mode != 0 && pivot_mode != 1))
        return ORBX_ERR_ARG;
    E* d = nullptr;
    if (hipMalloc(&d, 4 * sizeof(E) * (n + 8)) != hipSuccess) return ORBX_ERR_NOMEM;
    int r = ORBX_OK;
    if (hipMemcpy(d, entries, sizeof(E) * n, hipMemcpyHostToDevice) != hipSuccess) r = ORBX_ERR_HIP;
    if (r == ORBX_OK) {
        hipLaunchKernelGGL(k_debug_nth<E>, dim3(1), dim3(64), 0, 0, d, n, nth, d + (n + 8), d + 2 * (n + 8),
                           reinterpret_cast<int*>(d + 3 * (n + 8)), pivot_mode);
        if (hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(out_glb, d + (n + 8), sizeof(E) * n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out_lds, d + 2 * (n + 8), sizeof(E) * n, hipMemcpyDeviceToHost) != hipSuccess)
            r = ORBX_ERR_HIP;
    }
    (void)hipFree(d);
    return r;
}

}  // namespace orbx

extern "C" int orbx_debug_nth_pivot(const uint32_t* entries, int n, int nth, int pivot_mode, uint32_t* out_glb,
                                    uint32_t* out_lds)
{
    return orbx::debug_nth(entries, n, nth, pivot_mode, out_glb, out_lds);
}

// Harris-keyed entries, as k_harris_cells builds them: harris_key(response) << 32 | index
extern "C" int orbx_debug_nth64(const float* responses, int n, int nth, int pivot_mode, uint64_t* out_glb,
                                uint64_t* out_lds)
{
    if (!responses || n < 0 || n > orbx::kRetainCellCap) return ORBX_ERR_ARG;
    std::vector<uint64_t> e((size_t)n);
    for (int i = 0; i < n; i++) e[i] = (uint64_t)orbx::harris_key(responses[i]) << 32 | (uint32_t)i;
    static const uint64_t none = 0;
    return orbx::debug_nth(n ? e.data() : &none, n, nth, pivot_mode, out_glb, out_lds);
}

extern "C" int orbx_debug_nth(const uint32_t* entries, int n, int nth, uint32_t* out_glb, uint32_t* out_lds)
{
    return orbx_debug_nth_pivot(entries, n, nth, ORBX_NTH_PIVOT_GCC48, out_glb, out_lds);   // the default era
}

namespace orbx {

// Test hook: k_describe's window staging and patch blur for one position of
// one level, both halves of the wave on the same keypoint; the blurred 37x37
// patch goes to out, row-major.  lev / stride: the level as k_describe sees
// it (level_src).
__global__ __launch_bounds__(64) void k_debug_describe_patch(const uint8_t* lev, int stride, LevelGeom L,
                                                             int X, int Y, uint8_t* out)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_patch[2][kDescWaveBytes];
    const int lane = threadIdx.x, half = lane >> 5, hl = lane & 31;
    uint8_t* win = s_patch[half] + kWinPad;
    const int centre = describe_stage_window(lev, (uint32_t)stride, L.w, L.h, X, Y, win, hl);
    wave_lds_sync();
    describe_blur_window(win, X, Y, L.w, L.h, L.nvec_blur, hl);
    if (half == 0)
        for (int i = hl; i < kBrRows * kBrRows; i += 32) {
            const int r = i / kBrRows, c = i - r * kBrRows;
            out[i] = win[centre + (r - kBrR) * kBrPitch + (c - kBrR)];
        }
}

// Test hook: k_describe's window staging and IC_Angle moments for one position
// of one level, both halves of the wave on the same keypoint; out: m01, m10 of
// half 0, then of half 1.
__global__ __launch_bounds__(64) void k_debug_describe_moments(const uint8_t* lev, int stride, LevelGeom L,
                                                               const uint32_t* ic_rows, int X, int Y, int* out)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_patch[2][kDescWaveBytes];
    const int lane = threadIdx.x, half = lane >> 5, hl = lane & 31;
    uint8_t* win = s_patch[half] + kWinPad;
    uint32_t icw[kIcTabDw];
    describe_ic_weights(ic_rows, hl, icw);
    describe_stage_window(lev, (uint32_t)stride, L.w, L.h, X, Y, win, hl);
    wave_lds_sync();
    int m01, m10;
    describe_moments(win, X, hl, icw, m01, m10);
    if (hl == 0) {
        out[2 * half] = m01;
        out[2 * half + 1] = m10;
    }
}

// k_pyr_level0 over nb frames on stream st (x: levels, frames, first_slot,
// pyr_raw, w, h).
static void launch_level0(const Geometry& g, const ExtractArgs& x, int nb, hipStream_t st)
{
    const LevelGeom& L = g.levels[0];
    // interior 16-byte words: two aligned source loads cover them
    // (frames rows are 16-byte aligned when w % 16 == 0)
    const int qpr = L.stride / 16;
    int q_lo = (kEdge + 15) / 16, q_hi = (L.w + kEdge + kPyr0Shift - 32) / 16;
    q_hi = std::min(q_hi, qpr - 1);
    const int nint = (g.w % 16 == 0 && q_hi >= q_lo) ? q_hi - q_lo + 1 : 0;
    if (nint == 0) q_lo = 0;
    const int items = nint * ((L.ph + kPyrRows - 1) / kPyrRows) + (qpr - nint) * L.ph;
    hipLaunchKernelGGL(k_pyr_level0, dim3((items + 255) / 256, nb), dim3(256), 0, st, x, q_lo, nint);
}

// The padded level 0 of one slot, from the slot's current frame, on the
// context stream.  Extraction in direct mode leaves the area unwritten, so
// the readers of the padded level (orbx_dev_read_level, the whole-level blur)
// call this first; the copy depends on the frame alone, so it is repeated
// rather than tracked per slot.
int launch_level0_slot(orbx_ctx* ctx, int slot)
{
    ExtractArgs a = {};
    a.levels = ctx->dgeom.levels;
    a.frames = ctx->frames;
    a.first_slot = slot;
    a.pyr_raw = ctx->pyr_raw + (size_t)slot * ctx->geom.frame_pyr_bytes;
    a.frame_pyr_bytes = ctx->geom.frame_pyr_bytes;
    a.w = ctx->geom.w;
    a.h = ctx->geom.h;
    launch_level0(ctx->geom, a, 1, ctx->stream);
    if (hipGetLastError() != hipSuccess) return ORBX_ERR_HIP;
    return ORBX_OK;
}

// The borders of levels 1 .. nlevels - 1 of one frame's pyramid (pyr), as
// copyMakeBorder(BORDER_REFLECT_101) of the level leaves them: one thread per
// dword of the padded rows that is not wholly interior; each of its bytes
// inside the padded width is the interior byte its position reflects to, the
// row padding behind it zero.  Interior bytes are only read (a word that
// straddles the interior's edge stores its interior bytes back unchanged).
__global__ __launch_bounds__(256) void k_pyr_borders(const LevelGeom* levels, uint8_t* pyr)
{
    const LevelGeom L = cget(levels, 1 + (int)blockIdx.y);
    const int nq = L.stride >> 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nq * L.ph) return;
    const int py = idx / nq, p0 = 4 * (idx - py * nq);
    if (py >= kEdge && py < kEdge + L.h && p0 >= kEdge && p0 + 4 <= kEdge + L.w) return;
    uint8_t* lev = pyr + L.off;
    const uint8_t* src = lev + (size_t)(kEdge + reflect101(py - kEdge, L.h)) * L.stride + kEdge;
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (p0 + b < L.pw) word |= (uint32_t)src[reflect101(p0 + b - kEdge, L.w)] << (8 * b);
    *reinterpret_cast<uint32_t*>(lev + (size_t)py * L.stride + p0) = word;
}

// The batch resize (k_pyr_resize_lds) leaves the borders of levels >= 1
// unwritten, so the readers of a padded level (orbx_dev_read_level, the
// whole-level blur) call this first, on the context stream and after the
// slot's pyramid; the fill depends on the level interiors alone, so it is
// repeated rather than tracked per slot.  Where the borders were written
// (the single-frame cascade, k_pyr_resize) it stores the same bytes again.
int launch_borders_slot(orbx_ctx* ctx, int slot)
{
    const Geometry& g = ctx->geom;
    if (g.nlevels < 2) return ORBX_OK;
    const LevelGeom& L = g.levels[1];   // the largest of the levels filled
    const int items = (L.stride / 4) * L.ph;
    hipLaunchKernelGGL(k_pyr_borders, dim3((items + 255) / 256, g.nlevels - 1), dim3(256), 0, ctx->stream,
                       ctx->dgeom.levels, ctx->pyr_raw + (size_t)slot * g.frame_pyr_bytes);
    if (hipGetLastError() != hipSuccess) return ORBX_ERR_HIP;
    return ORBX_OK;
}

// The whole-level blur of one slot's raw pyramid into the one-frame
// ctx->pyr_blur, on the context stream (orbx_dev_read_level's blurred levels).
int launch_blur_slot(orbx_ctx* ctx, int slot)
{
    const int r0 = launch_level0_slot(ctx, slot);   // k_blur reads the padded level 0
    if (r0 != ORBX_OK) return r0;
    const int r1 = launch_borders_slot(ctx, slot);  // and the borders of the levels above it
    if (r1 != ORBX_OK) return r1;
    ExtractArgs a = {};
    a.levels = ctx->dgeom.levels;
    a.pyr_raw = ctx->pyr_raw + (size_t)slot * ctx->geom.frame_pyr_bytes;
    a.pyr_blur = ctx->pyr_blur;
    a.frame_pyr_bytes = ctx->geom.frame_pyr_bytes;
    hipLaunchKernelGGL(k_blur, dim3(ctx->blur_tiles_n, 1), dim3(kBlurItems), 0, ctx->stream, a, ctx->blur_tiles);
    if (hipGetLastError() != hipSuccess) return ORBX_ERR_HIP;
    return ORBX_OK;
}

}  // namespace orbx

/* Diagnostics (not in include/orbx.h): the blurred 37x37 descriptor patch
 * that k_describe builds for a keypoint at level position (x, y) of slot
 * `slot`'s raw pyramid, 16 <= x < w - 16, 16 <= y < h - 16, row-major. */
extern "C" int orbx_debug_describe_patch(orbx_ctx* ctx, int slot, int level, int x, int y, uint8_t* out)
{
    using namespace orbx;
    if (!ctx || !out || slot < 0 || slot >= ctx->slots || level < 0 || level >= ctx->geom.nlevels) return ORBX_ERR_ARG;
    const LevelGeom& L = ctx->geom.levels[level];
    if (x < kEdge || x >= L.w - kEdge || y < kEdge || y >= L.h - kEdge) return ORBX_ERR_ARG;
    ctx_enter(ctx);
    uint8_t* d = nullptr;
    if (hipDeviceSynchronize() != hipSuccess) return ORBX_ERR_HIP;   // every part stream's pyramid
    if (hipMalloc(&d, kBrRows * kBrRows) != hipSuccess) return ORBX_ERR_NOMEM;
    // the level as k_describe sees it: level 0 of frames that qualify for the
    // direct mode is the slot's frame (its virtual padded origin, level_src);
    // the padded level 0 of such a slot may never have been written, and
    // where the cascade wrote it, it holds the same bytes
    const bool direct = level == 0 && kEdge == 16 && ctx->geom.w % 16 == 0;
    const long long fw = ctx->geom.w, fh = ctx->geom.h;
    const uint8_t* lev = direct ? ctx->frames + ((long long)slot * fw * fh - (long long)kEdge * fw - kEdge)
                                : ctx->pyr_raw + (size_t)slot * ctx->geom.frame_pyr_bytes + L.off;
    hipLaunchKernelGGL(k_debug_describe_patch, dim3(1), dim3(64), 0, ctx->stream, lev, direct ? (int)fw : L.stride,
                       L, kEdge + x, kEdge + y, d);
    int r = ORBX_OK;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(out, d, kBrRows * kBrRows, hipMemcpyDeviceToHost) != hipSuccess)
        r = ORBX_ERR_HIP;
    (void)hipFree(d);
    return r;
}

/* Diagnostics (not in include/orbx.h): IC_Angle's moments as k_describe
 * computes them for a keypoint at level position (x, y) of slot `slot`'s raw
 * pyramid (the same range as above): out = m01, m10 of the wave's lower half,
 * then of its upper half, both on the same keypoint. */
extern "C" int orbx_debug_describe_moments(orbx_ctx* ctx, int slot, int level, int x, int y, int32_t* out)
{
    using namespace orbx;
    if (!ctx || !out || slot < 0 || slot >= ctx->slots || level < 0 || level >= ctx->geom.nlevels) return ORBX_ERR_ARG;
    const LevelGeom& L = ctx->geom.levels[level];
    if (x < kEdge || x >= L.w - kEdge || y < kEdge || y >= L.h - kEdge) return ORBX_ERR_ARG;
    ctx_enter(ctx);
    int* d = nullptr;
    if (hipDeviceSynchronize() != hipSuccess) return ORBX_ERR_HIP;   // every part stream's pyramid
    if (hipMalloc(&d, 4 * sizeof(int)) != hipSuccess) return ORBX_ERR_NOMEM;
    // the level as k_describe sees it (see orbx_debug_describe_patch)
    const bool direct = level == 0 && kEdge == 16 && ctx->geom.w % 16 == 0;
    const long long fw = ctx->geom.w, fh = ctx->geom.h;
    const uint8_t* lev = direct ? ctx->frames + ((long long)slot * fw * fh - (long long)kEdge * fw - kEdge)
                                : ctx->pyr_raw + (size_t)slot * ctx->geom.frame_pyr_bytes + L.off;
    hipLaunchKernelGGL(k_debug_describe_moments, dim3(1), dim3(64), 0, ctx->stream, lev, direct ? (int)fw : L.stride,
                       L, ctx->dgeom.ic_rows, kEdge + x, kEdge + y, d);
    int r = ORBX_OK;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(out, d, 4 * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        r = ORBX_ERR_HIP;
    (void)hipFree(d);
    return r;
}

/* Diagnostics (not in include/orbx.h): fills the whole raw-pyramid area of
 * slots [first_slot, first_slot + count) with one byte value, after every
 * pending launch and before every later one (tests poison the areas to show
 * that no result depends on bytes the extraction does not write). */
extern "C" int orbx_debug_fill_pyramid(orbx_ctx* ctx, int first_slot, int count, int byte)
{
    if (!ctx || first_slot < 0 || count < 0 || first_slot + count > ctx->slots || !ctx->pyr_raw) return ORBX_ERR_ARG;
    ctx_enter(ctx);
    if (hipDeviceSynchronize() != hipSuccess) return ORBX_ERR_HIP;   // every part stream's work on the slots
    const size_t fb = (size_t)ctx->geom.frame_pyr_bytes;
    if (count > 0 && fb > 0 &&
        hipMemsetAsync(ctx->pyr_raw + (size_t)first_slot * fb, byte & 0xFF, (size_t)count * fb, ctx->stream) != hipSuccess)
        return ORBX_ERR_HIP;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return ORBX_ERR_HIP;
    return ORBX_OK;
}

/* Diagnostics (not in include/orbx.h): 1 when the last extraction launched on
 * the context read level 0 from the frame store (no k_pyr_level0 copy), else 0. */
extern "C" int orbx_debug_level0_direct(orbx_ctx* ctx)
{
    if (!ctx) return ORBX_ERR_ARG;
    return ctx->last_l0_direct ? 1 : 0;
}

/* Diagnostics (not in include/orbx.h): the k_fast_cells instance that the last
 * extraction launched on the context: out[0] the compile-time tile pitch (0:
 * the runtime-pitch instance), out[1] the workgroup's threads, out[2] the band
 * rows (0: whole cells).  ORBX_ERR_ARG before the first extraction. */
extern "C" int orbx_debug_fast_instance(orbx_ctx* ctx, int* out)
{
    if (!ctx || !out || ctx->last_fast[0] < 0) return ORBX_ERR_ARG;
    for (int k = 0; k < 3; k++) out[k] = ctx->last_fast[k];
    return ORBX_OK;
}

/* Diagnostics (not in include/orbx.h): the capacity (entries) of k_fast_cells'
 * scored-pixel list for the context's later extractions; n < 0 restores the
 * default, 0 sends every cell down the dword path.  A launch without LDS for
 * it runs with capacity 0 whatever is set.  Set it before the context's first
 * orbx_extract (whose captured graph keeps the launch's arguments). */
extern "C" int orbx_debug_fast_list_cap(orbx_ctx* ctx, int n)
{
    if (!ctx) return ORBX_ERR_ARG;
    ctx->fast_list_cap = n < 0 ? -1 : n;
    return ORBX_OK;
}

/* Diagnostics (not in include/orbx.h): per cell of slot `slot`'s last
 * extraction, the paths its bands took through NMS and emission (bit 0: the
 * scored-pixel list, bit 1: the dword path; 0: nothing scored, an invalid
 * cell or one without interior rows); *list_cap gets the capacity the last
 * launch ran with.  Returns the number of cells. */
extern "C" int orbx_debug_fast_paths(orbx_ctx* ctx, int slot, uint8_t* out, int cap, int* list_cap)
{
    if (!ctx || !out || !list_cap || slot < 0 || slot >= ctx->slots || ctx->last_fast[0] < 0) return ORBX_ERR_ARG;
    ctx_enter(ctx);
    const orbx::Geometry& g = ctx->geom;
    const int n = (int)g.cells.size();
    if (cap < n) return ORBX_ERR_CAPACITY;
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(out, ctx->fast_path + (size_t)slot * n, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
        return ORBX_ERR_HIP;
    for (int c = 0; c < n; c++)
        if (!g.cells[c].valid) out[c] = 0;
    *list_cap = ctx->last_fast[3];
    return n;
}

/* Diagnostics (not in include/orbx.h): FAST's output for slot `slot` of the
 * last extraction, before retainBest: per cell 10 ints in `cells` (level,
 * ini_x, ini_y, hx, hy, valid, list offset, list capacity, corner count, 0)
 * and the slot's corner arena in `lists` (entry: S << 24 | level y << 12 |
 * level x, each cell's corners in raster order from its list offset).
 * Returns the number of cells; *entries gets the arena's length. */
extern "C" int orbx_debug_fast_lists(orbx_ctx* ctx, int slot, int32_t* cells, int cells_cap, uint32_t* lists,
                                     int lists_cap, int* entries)
{
    using namespace orbx;
    if (!ctx || !cells || !lists || !entries || slot < 0 || slot >= ctx->slots) return ORBX_ERR_ARG;
    ctx_enter(ctx);
    const Geometry& g = ctx->geom;
    const int n = (int)g.cells.size();
    if (cells_cap < 10 * n || lists_cap < g.list_entries) return ORBX_ERR_CAPACITY;
    std::vector<int32_t> cnt(n);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(cnt.data(), ctx->cell_count + (size_t)slot * n, 4 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(lists, ctx->cell_lists + (size_t)slot * g.list_entries, 4 * (size_t)g.list_entries,
                  hipMemcpyDeviceToHost) != hipSuccess)
        return ORBX_ERR_HIP;
    for (int c = 0; c < n; c++) {
        const CellGeom& C = g.cells[c];
        const int32_t v[10] = {C.level, C.ini_x, C.ini_y, C.hx, C.hy, C.valid ? 1 : 0, C.list_off, C.list_cap, cnt[c], 0};
        for (int k = 0; k < 10; k++) cells[10 * c + k] = v[k];
    }
    *entries = g.list_entries;
    return n;
}

namespace orbx {

// ---------------------------------------------------------------------------
// Host launcher
// ---------------------------------------------------------------------------
int launch_extract(orbx_ctx* ctx, int first, int count, const MatchSpec* m)
{
    const Geometry& g = ctx->geom;
    if (count > 1 || (m && m->kind != 0 && ctx->async_match)) {   // the batch pipeline's streams
        const int r = ensure_aux_streams(ctx);
        if (r != ORBX_OK) return r;
    }
    for (int sl = first; sl < first + count && sl < (int)ctx->bow_ready.size(); sl++) ctx->bow_ready[sl] = 0;
    // frames still being uploaded (orbx_dev_upload_async): every part and
    // half below starts on, or is released from, the context stream
    wait_uploads_overlap(ctx, first, count, ctx->stream);
    ExtractArgs a;
    a.levels = ctx->dgeom.levels;
    a.cells = ctx->dgeom.cells;
    a.res_cols = ctx->dgeom.res_cols;
    a.res_rows = ctx->dgeom.res_rows;
    a.ic_rows = ctx->dgeom.ic_rows;
    a.frames = ctx->frames;
    // work buffers are per slot (frame f of this pass uses slot first + f):
    // batches on disjoint slots can be in flight at the same time
    a.pyr_raw = ctx->pyr_raw + (size_t)first * g.frame_pyr_bytes;
    a.pyr_blur = nullptr;   // off the extraction path (launch_blur_slot fills the one-frame buffer)
    a.cell_lists = ctx->cell_lists + (size_t)first * g.list_entries;
    a.cell_count = ctx->cell_count + (size_t)first * g.cells.size();
    a.fast_path = ctx->fast_path;
    a.level_keys = ctx->level_keys + (size_t)first * g.level_entries;
    a.level_count = ctx->level_count + (size_t)first * g.nlevels;
    a.out_kps = ctx->out_kps;
    a.out_desc = ctx->out_desc;
    a.out_n = ctx->out_n;
    a.error_flags = ctx->error_flags;
    a.host_out = ctx->single_frame ? ctx->single_out : nullptr;
    a.retain_scratch = ctx->retain_scratch + (size_t)first * (g.list_entries + 4 * g.cells.size());
    a.harris = ctx->harris;
    a.fp_contract = ctx->fp_contract;
    a.nth_pivot = ctx->nth_pivot;
    // the level retain holds a whole level list (+ scratch) in one block's LDS
    if ((size_t)((ctx->harris ? 3 : 2) * g.max_level_cap + 8) * 4 > 160 * 1024) return ORBX_ERR_UNSUPPORTED;
    a.cell_keys64 = ctx->harris ? ctx->cell_keys64 + (size_t)first * g.list_entries : nullptr;
    a.level_keys64 = ctx->harris ? ctx->level_keys64 + (size_t)first * g.level_entries : nullptr;
    a.frame_pyr_bytes = g.frame_pyr_bytes;
    a.w = g.w;
    a.h = g.h;
    a.nlevels = g.nlevels;
    a.ncells = (int)g.cells.size();
    a.list_entries = g.list_entries;
    a.level_entries = g.level_entries;
    a.nfeatures = g.nfeatures;
    a.fast_th = min(max(g.fast_th, 0), 255);
    a.fast_th_low = 7;
    a.max_list_cap = g.max_list_cap;
    a.max_level_cap = g.max_level_cap;
    // Level 0 straight from the frame store (level_src), without the padded
    // copy: rows of w % 16 == 0 bytes keep the kernels' 16-byte loads
    // aligned; the single-frame cascade writes level 0 itself.  A slot's frame
    // is then read until its k_describe ends: whatever overwrites frames is
    // ordered after the whole queued extraction.
    a.l0_direct = (kEdge == 16 && g.w % 16 == 0 && !(ctx->single_frame && g.cascade_bands > 0)) ? 1 : 0;
    ctx->last_l0_direct = a.l0_direct != 0;

    // The pyramid stages over nb frames on stream st.
    auto run_pyramid = [&](const ExtractArgs& x, int nb, hipStream_t st) {
        // orbx_extract's single-frame graph: the whole raw pyramid in one
        // launch (its lowest latency; batches fill the chip with the staged
        // per-level launches below, which measured faster there)
        if (ctx->single_frame && g.cascade_bands > 0) {
            timer_begin(ctx, "resize", st);
            for (int rep = 0; rep < kDiagRepeat[0]; rep++) {
                {
                    int tab_off = (g.cascade_lds + 15) & ~15;
                    size_t lds = (size_t)tab_off + 8 * (size_t)(g.cascade_tab_cols + g.cascade_tab_rows);
                    if (lds > 160 * 1024) {   // very wide frames: the tables stay in HBM
                        tab_off = 0;
                        lds = g.cascade_lds;
                    }
                    hipLaunchKernelGGL(k_pyr_cascade<ORBX_CASCADE_SINGLE_THREADS>, dim3(g.cascade_bands, nb),
                                       dim3(ORBX_CASCADE_SINGLE_THREADS), lds, st, x, ctx->cascade, g.cascade_buf_x,
                                       tab_off, g.cascade_tab_cols);
                }
            }
            timer_end(ctx, "resize", st);
            return;
        }
        if (!x.l0_direct) {   // direct mode: no launch, and the "pyr0" timer reports none
            timer_begin(ctx, "pyr0", st);
            launch_level0(g, x, nb, st);
            timer_end(ctx, "pyr0", st);
        }
        for (int l = 1; l < g.nlevels; l++) {
            const LevelGeom& L = g.levels[l];
            const LevelGeom& P = g.levels[l - 1];
            // staged parent rows: from the first interior byte, in the padded
            // level as in the frame (the direct level 0)
            const int pitch = (P.w + 15) & ~15;
            const size_t lds = (size_t)L.res_span * pitch + (size_t)L.w * sizeof(ResizeCol);
            timer_begin(ctx, "resize", st);
            if (lds <= kResizeLds) {
                const int threads = std::min(256, ((L.stride / 4) + 63) & ~63);
                // the packed form needs each interior word's taps within 8
                // bytes (source step < 2 keeps them within 7; a level just
                // over 2x, e.g. 333 -> 166, may not)
                int packed = 1;
                for (int x0 = 0; x0 + 3 < L.w; x0 += 4)
                    if (g.res_cols[L.res_col_off + x0 + 3].sx0 - g.res_cols[L.res_col_off + x0].sx0 > 6) packed = 0;
                // interior words of the packed form (k_pyr_resize_lds's nfast):
                // whole waves slide down the strip; a remainder of at most 32
                // words shares one wave as 64 / rem row groups
                const int q_lo = (kEdge + 3) >> 2;
                const int nfast = packed ? std::max(q_lo, (kEdge + std::min(L.w, L.nvec_resize)) >> 2) - q_lo : 0;
                int nslide = nfast, rem_wave = 0, rem_n = 0;
                if (const int rem = nfast & 63; rem > 0 && rem <= 32) {
                    nslide = nfast - rem;
                    rem_wave = (nslide >> 6) % (threads >> 6);
                    const int groups = 64 / rem;
                    rem_n = (kResRows + groups - 1) / groups;
                }
                const ResizeLevel rl{L.off, P.off, L.stride, P.stride, L.w, L.h, P.h, L.nvec_resize,
                                     L.res_span, L.res_strip_off, L.res_row_off, L.res_col_off, packed, l - 1,
                                     nslide, rem_wave, rem_n};
                // one workgroup per strip of interior rows (no border rows)
                for (int rep = 0; rep < kDiagRepeat[0]; rep++)
                    hipLaunchKernelGGL(k_pyr_resize_lds, dim3((L.h + kResRows - 1) / kResRows, nb), dim3(threads), lds,
                                       st, x, rl, pitch);
            } else {   // very wide levels: per-pixel gathers from global memory
                const int items = (L.stride / 4) * ((L.ph + kPyrRows - 1) / kPyrRows);
                hipLaunchKernelGGL(k_pyr_resize, dim3((items + 255) / 256, nb), dim3(256), 0, st, x, l);
            }
            timer_end(ctx, "resize", st);
        }
    };
    // FAST .. describe over nb frames on stream st (after their pyramid).
    // parts: 1 = FAST, 2 = retain, 8 = describe (4 was the whole-level blur:
    // k_describe blurs its own patches)
    auto run_rest = [&](const ExtractArgs& x, int nb, hipStream_t st, int parts) {
        if (parts & 1) {
        timer_begin(ctx, "fast", st);
        {
            // widest aligned cell row and tallest cell pick the tile pitch
            int wmax = 0, hmax = 0;
            for (const CellGeom& c : g.cells) {
                if (!c.valid) continue;
                wmax = std::max(wmax, (15 + c.hx + 15) & ~15);
                hmax = std::max(hmax, c.hy);
            }
            const dim3 grid((int)g.cells.size(), nb);
            // Whole cells when a workgroup's LDS (tile + S' + nz + the static
            // survivor queues) stays within kFastLdsTarget (4 workgroups per
            // CU); taller cells are split into the fewest equal row bands
            // whose windows (band + 8 halo rows) fit.
            auto plan = [&](int P, int static_lds, int& band_rows) {
                band_rows = 0;
                const int whole = fast_tile_bytes(hmax, P);
                if (fast_lds_bytes(whole) + static_lds <= kFastLdsTarget || hmax <= 9) return whole;
                int wh = hmax;
                while (wh > 9 && fast_lds_bytes(fast_tile_bytes(wh, P)) + static_lds > kFastLdsTarget) wh--;
                const int nint = hmax - 6, bmax = wh - 8;
                const int nbands = (nint + bmax - 1) / bmax;
                band_rows = (nint + nbands - 1) / nbands;
                return fast_tile_bytes(std::min(hmax, band_rows + 8), P);
            };
            auto fast = [&](auto kern, int pitch, int bytes, int band_rows, int threads) {
                const int lds = fast_lds_bytes(bytes);
                ctx->last_fast[0] = pitch;
                ctx->last_fast[1] = threads;
                ctx->last_fast[2] = band_rows;
                // The scored-pixel list and its kept bitmap go behind the
                // planned bytes where the workgroup stays within the target
                // (and the bitmap's u16 prefix table fits the queues' 3 KB);
                // else capacity 0: every cell on the dword path.
                const bool u32e = pitch == 0;
                int cap = ctx->fast_list_cap < 0 ? kFastListCap : std::min(ctx->fast_list_cap, 4096);
                if (cap > 0 && (lds + fast_static_lds(u32e) + fast_list_lds(bytes, cap, u32e) > kFastLdsTarget || bytes / 32 > 1536))
                    cap = 0;
                ctx->last_fast[3] = cap;
                hipLaunchKernelGGL(kern, grid, dim3(threads), lds + fast_list_lds(bytes, cap, u32e), st, x, bytes, band_rows,
                                   cap);
            };
            // the templated instances queue u16 tile positions: windows of up
            // to 64 KB (larger ones take the runtime-pitch instance)
            // whole cells at the 96 / 144 / 208 pitches (their tiles fit four
            // workgroups per CU at the frame sizes of interest), row bands
            // where needed at 336 (1920x1080) and the runtime pitch
            int br = 0, bytes = 0;
            auto fits = [&](int P) {
                if (wmax > P) return false;
                bytes = fast_tile_bytes(hmax, P);
                return bytes <= 65536;
            };
            auto fits_banded = [&](int P) {
                if (wmax > P) return false;
                bytes = plan(P, fast_static_lds(false), br);
                return bytes <= 65536;
            };
            if (fits(96)) fast(k_fast_cells<96>, 96, bytes, 0, 256);
            else if (fits(144)) {
                for (int rep = 0; rep < kDiagRepeat[3]; rep++) fast(k_fast_cells<144>, 144, bytes, 0, 256);
            } else if (fits(208)) fast(k_fast_cells<208>, 208, bytes, 0, 256);
            else if (fits_banded(336))
                fast(k_fast_cells<336, kFastWideThreads, true>, 336, bytes, br, kFastWideThreads);
            else {
                bytes = plan(wmax, fast_static_lds(true), br);
                fast(k_fast_cells<0, kFastWideThreads, true>, 0, bytes, br, kFastWideThreads);
            }
        }
        timer_end(ctx, "fast", st);
        }
        if (parts & 2) {
        timer_begin(ctx, "retain", st);
        {
            // wave-private LDS (u32 words): cell list + partition scratch
            // (longer lists are replayed in global memory)
            const int ew = x.harris ? 2 : 1;   // u32 words per entry
            const int cw = (ew + 1) * kRetainCellCap + 8;
            const int cwaves = 4;
            const int lw = (ew + 1) * g.max_level_cap + 8;
            const int lwaves = 1;   // one level per block: small LDS blocks fit beside the other stream's kernels
            const dim3 cgrid(((int)g.cells.size() + cwaves - 1) / cwaves, nb), lgrid((g.nlevels + lwaves - 1) / lwaves, nb);
            if (x.harris) {
                hipLaunchKernelGGL(k_harris_cells, dim3((int)g.cells.size(), nb), dim3(256), 0, st, x);
                hipLaunchKernelGGL(k_retain_cells<uint64_t>, cgrid, dim3(64 * cwaves), (size_t)cwaves * cw * 4, st, x,
                                   cwaves, cw);
                hipLaunchKernelGGL(k_retain_levels<uint64_t>, lgrid, dim3(64 * lwaves), (size_t)lwaves * lw * 4, st, x,
                                   lwaves, lw);
            } else {
                hipLaunchKernelGGL(k_retain_cells<uint32_t>, cgrid, dim3(64 * cwaves), (size_t)cwaves * cw * 4, st, x,
                                   cwaves, cw);
                hipLaunchKernelGGL(k_retain_levels<uint32_t>, lgrid, dim3(64 * lwaves), (size_t)lwaves * lw * 4, st, x,
                                   lwaves, lw);
            }
        }
        timer_end(ctx, "retain", st);
        }
        if (!(parts & 8)) return;
        timer_begin(ctx, "describe", st);
        const dim3 dgrid((g.nfeatures + 2 * kWaves - 1) / (2 * kWaves), xcd_frames(nb));
        for (int rep = 0; rep < kDiagRepeat[2]; rep++) {
            if (x.fp_contract)
                hipLaunchKernelGGL(k_describe<true>, dgrid, dim3(256), 0, st, x, nb);
            else
                hipLaunchKernelGGL(k_describe<false>, dgrid, dim3(256), 0, st, x, nb);
        }
        timer_end(ctx, "describe", st);
    };
    auto run = [&](const ExtractArgs& x, int nb, hipStream_t st) {
        run_pyramid(x, nb, st);
        run_rest(x, nb, st, 15);
    };
    // Matching of slot s against prev(s) (the rule of orbx_dev_match_prev),
    // for the slots of [lo, hi) whose predecessor lies in [plo, phi) (all of
    // them when phi < 0), launched as contiguous runs on stream st.
    int err = ORBX_OK;
    auto match_runs = [&](int lo, int hi, int plo, int phi, hipStream_t st) {
        if (!m || m->kind == 0) return;
        auto prev = [&](int sl) { return (sl % m->seq_len == 0) ? sl + m->seq_len - 1 : sl - 1; };
        auto take = [&](int sl) {
            const int p = prev(sl);
            return phi < 0 || (p >= plo && p < phi);
        };
        for (int s0 = lo; s0 < hi;) {
            if (!take(s0)) {
                s0++;
                continue;
            }
            int s1 = s0 + 1;
            while (s1 < hi && take(s1)) s1++;
            const int r = m->kind == 1 ? launch_match_prev(ctx, s0, s1 - s0, m->seq_len, m->window, m->nnratio,
                                                           m->check_ori, st)
                                       : launch_match_bf_prev(ctx, s0, s1 - s0, m->seq_len, m->th_low, m->nnratio, st);
            if (r != ORBX_OK) err = r;
            s0 = s1;
        }
    };
    // Every buffer is indexed by slot: the frame store and outputs, and the
    // work buffers too (a.pyr_raw, cell_lists, retain_scratch, the key lists
    // are offset by `first`, and by a part's first slot below), so calls on
    // disjoint slot ranges never share scratch.  Parts launched on stream2 /
    // xstreams are never joined back to ctx->stream: later calls are ordered
    // after them only through the pending-match events that ctx_enter and
    // wait_pending_overlap wait on (the match stream waits for every part).
    // Large batches run
    // as two halves on two streams so that the VALU-bound FAST pass of one
    // half overlaps the latency-bound passes of the other; each half's
    // internal frame pairs are matched on its own stream, the pairs that
    // straddle the halves after the join.
    a.first_slot = first;
    const bool async = m && m->kind != 0 && ctx->async_match && ctx->mstream;
    // outputs of [first, first + count) are rewritten: a pending match that
    // reads any of them must finish first
    if (!async) {
        wait_pending_overlap(ctx, first, count, ctx->stream);
        ctx->stream_dirty = true;
    }
    if (async) {
        // Extraction, then the batch's matching on mstream, which overlaps
        // the next call's extraction of other slots.  Batches large enough
        // to split run as a software pipeline over two streams: the first
        // half's pyramid + FAST on the context stream, then its retain ..
        // describe while the second half (stream2, started at that point)
        // runs its pyramid + FAST; the next call's first half follows on the
        // context stream during the second half's tail.  The VALU-bound FAST
        // of one half thus overlaps the latency-bound stages of the other,
        // in steady state.  mstream's match waits for both halves.
        const int ways = std::min(ctx->split_ways, count / kSplitMinFrames);
        if (ctx->split && ways >= 2 && ctx->stream2) {
            // outputs of [first, first + count) are rewritten: pending matches
            // reading them finish first (the other parts' streams inherit it
            // through the release chain)
            wait_pending_overlap(ctx, first, count, ctx->stream);
            const hipStream_t S[orbx_ctx::kMaxWays] = {ctx->stream, ctx->stream2, ctx->xstreams[0], ctx->xstreams[1]};
            for (int i = 0; i < ways; i++) {
                const int lo = count * i / ways, n = count * (i + 1) / ways - lo;
                ExtractArgs b = a;
                b.first_slot = first + lo;
                b.pyr_raw += (size_t)lo * a.frame_pyr_bytes;
                b.cell_lists += (size_t)lo * a.list_entries;
                b.retain_scratch += (size_t)lo * (a.list_entries + 4 * a.ncells);
                b.cell_count += (size_t)lo * a.ncells;
                b.level_keys += (size_t)lo * a.level_entries;
                if (a.harris) {
                    b.cell_keys64 += (size_t)lo * a.list_entries;
                    b.level_keys64 += (size_t)lo * a.level_entries;
                }
                b.level_count += (size_t)lo * a.nlevels;
                // part i starts once part i - 1 is past its FAST pass
                if (i > 0) ORBX_HIP_CHECK(hipStreamWaitEvent(S[i], ctx->ev_part_fast[i - 1], 0));
                run_pyramid(b, n, S[i]);
                run_rest(b, n, S[i], 1);
                ORBX_HIP_CHECK(hipEventRecord(ctx->ev_part_fast[i], S[i]));
                run_rest(b, n, S[i], 14);
                ORBX_HIP_CHECK(hipEventRecord(ctx->ev_part_done[i], S[i]));
                ORBX_HIP_CHECK(hipStreamWaitEvent(ctx->mstream, ctx->ev_part_done[i], 0));
            }
        } else {
            const int r = launch_extract(ctx, first, count, nullptr);
            if (r != ORBX_OK) return r;
            ORBX_HIP_CHECK(hipEventRecord(ctx->ev_extracted, ctx->stream));
            ORBX_HIP_CHECK(hipStreamWaitEvent(ctx->mstream, ctx->ev_extracted, 0));
        }
        match_runs(first, first + count, 0, -1, ctx->mstream);
        // the match reads the outputs of the batch's sequences
        const int q = m->seq_len;
        const int lo = (first / q) * q, hi = ((first + count + q - 1) / q) * q;
        ORBX_HIP_CHECK(push_pending(ctx, lo, hi));
        if (err != ORBX_OK) return err;
        if (hipGetLastError() != hipSuccess) return ORBX_ERR_HIP;
        return ORBX_OK;
    }
    if (ctx->split && count >= 2 * kSplitMinFrames && ctx->stream2) {
        const int n0 = count / 2, n1 = count - n0;
        ExtractArgs b = a;
        b.first_slot = first + n0;
        b.pyr_raw += (size_t)n0 * a.frame_pyr_bytes;
        b.cell_lists += (size_t)n0 * a.list_entries;
        b.retain_scratch += (size_t)n0 * (a.list_entries + 4 * a.ncells);
        b.cell_count += (size_t)n0 * a.ncells;
        b.level_keys += (size_t)n0 * a.level_entries;
        if (a.harris) {
            b.cell_keys64 += (size_t)n0 * a.list_entries;
            b.level_keys64 += (size_t)n0 * a.level_entries;
        }
        b.level_count += (size_t)n0 * a.nlevels;
        ORBX_HIP_CHECK(hipEventRecord(ctx->ev_fork, ctx->stream));
        ORBX_HIP_CHECK(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
        run(a, n0, ctx->stream);
        match_runs(first, first + n0, first, first + n0, ctx->stream);
        run(b, n1, ctx->stream2);
        match_runs(first + n0, first + count, first + n0, first + count, ctx->stream2);
        ORBX_HIP_CHECK(hipEventRecord(ctx->ev_join, ctx->stream2));
        ORBX_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        // straddling pairs (predecessor in the other half, or outside the batch)
        match_runs(first, first + n0, first + n0, 0x7fffffff, ctx->stream);
        match_runs(first, first + n0, -0x7fffffff, first, ctx->stream);
        match_runs(first + n0, first + count, first, first + n0, ctx->stream);
        match_runs(first + n0, first + count, first + count, 0x7fffffff, ctx->stream);
        match_runs(first + n0, first + count, -0x7fffffff, first, ctx->stream);
    } else if (ctx->single_frame && count == 1) {
        // one frame (orbx_extract's captured graph), for latency: the raw
        // pyramid as one cascade launch, then FAST, retain and describe
        run_pyramid(a, 1, ctx->stream);
        run_rest(a, 1, ctx->stream, 1 | 2 | 8);
        match_runs(first, first + count, 0, -1, ctx->stream);
    } else {
        run(a, count, ctx->stream);
        match_runs(first, first + count, 0, -1, ctx->stream);
    }
    if (err != ORBX_OK) return err;
    if (hipGetLastError() != hipSuccess) return ORBX_ERR_HIP;
    return ORBX_OK;
}


}  // namespace orbx
