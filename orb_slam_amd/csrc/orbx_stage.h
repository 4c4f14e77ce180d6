// Host-side staging of one call in the context scratch: where each array
// lies, and the three ways its bytes travel.
//
// A call lays its arrays out with take<T>(count).  The Region<T> it gets back
// is the only statement of that array's offset and length: the device pointer
// and every copy are derived from it.
//
// Layout (BlockStage, ArrayStage), for the matcher calls' few large arrays:
// every region starts on a 256-byte boundary and owns at least 256 bytes, so no
// two regions share an address, an empty one included.  BlockStage moves the
// call through the context's page-locked buffer: put / fill write at the
// region's own offset, one copy takes [0, end) up, one copy and a sync bring
// the read-back range down.  ArrayStage moves each array on its own between
// the caller's memory and the device.
//
// PackedStage (orbx_pack.h's PackedLayout), for the batched solver calls' ten
// small arrays per query: 16-byte granularity, a call-owned pageable blob, one
// upload; the result blocks behind the inputs come back through ResultBlocks.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "orbx_internal.h"
#include "orbx_pack.h"

namespace orbx {

inline size_t align256(size_t bytes) { return (bytes + 255) & ~size_t(255); }

struct Layout {
    size_t total = 0;
    template <typename T>
    Region<T> take(size_t count)
    {
        const Region<T> r{total, count};
        total += align256(std::max<size_t>(r.bytes(), 1));
        return r;
    }
};

// src/Frame.cc:98-102: mvScaleFactors
inline void level_scales(int nlevels, float scale_factor, float* out)
{
    out[0] = 1.0f;
    for (int i = 1; i < nlevels; i++) out[i] = out[i - 1] * scale_factor;
}

inline bool valid_frame_view(const orbx_frame_view* v)
{
    return v && v->n >= 0 && v->n <= kMaxFeatures && (v->n == 0 || (v->keys_un && v->desc)) && v->max_x > v->min_x &&
           v->max_y > v->min_y && v->nlevels > 0 && v->nlevels <= kMaxLevels;
}

// The whole call in the page-locked buffer `h`, which mirrors the scratch
// offset for offset: inputs (and initialised outputs) go over in ONE copy and
// the outputs come back in ONE copy, instead of a copy per array, each of
// which costs a DMA setup (and, from pageable memory, a staging kernel).  The
// standing order of a call's regions is
// [inputs | job structs | read-back range | device-only].
struct BlockStage : Layout {
    orbx_ctx* ctx;
    uint8_t* h = nullptr;
    explicit BlockStage(orbx_ctx* c) : ctx(c) {}
    // after the layout is complete; the pinned buffer reaches the end of the
    // read-back range (device-only regions have no host copy)
    int open(size_t readback_end)
    {
        int r = ensure_scratch(ctx, total);
        if (r == ORBX_OK) r = ensure_pinned(ctx, readback_end);
        if (r == ORBX_OK) h = static_cast<uint8_t*>(ctx->host_pinned);
        return r;
    }
    template <typename T>
    T* dev(Region<T> r) const
    {
        return region_ptr(ctx->scratch, r);
    }
    // the first `count` (<= r.count) elements
    template <typename T>
    void put(Region<T> r, const T* src, size_t count)
    {
        if (count && src) std::memcpy(h + r.off, src, count * sizeof(T));
    }
    template <typename T>
    void put(Region<T> r, const T* src)
    {
        put(r, src, r.count);
    }
    template <typename T>
    void fill(Region<T> r, int byte)
    {
        std::memset(h + r.off, byte, r.bytes());
    }
    template <typename T>
    void get(T* dst, Region<T> r, size_t count) const
    {
        if (count && dst) std::memcpy(dst, h + r.off, count * sizeof(T));
    }
    template <typename T>
    void get(T* dst, Region<T> r) const
    {
        get(dst, r, r.count);
    }
    int upload(size_t begin, size_t end)
    {
        ORBX_HIP_CHECK(hipMemcpyAsync(static_cast<uint8_t*>(ctx->scratch) + begin, h + begin, end - begin,
                                      hipMemcpyHostToDevice, ctx->stream));
        return ORBX_OK;
    }
    int upload(size_t end) { return upload(0, end); }
    int download(size_t begin, size_t end)
    {
        ORBX_HIP_CHECK(hipMemcpyAsync(h + begin, static_cast<uint8_t*>(ctx->scratch) + begin, end - begin,
                                      hipMemcpyDeviceToHost, ctx->stream));
        ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return ORBX_OK;
    }
};

// One copy per array between the caller's memory and the scratch.  An input
// named at take() goes up in upload(), in the order taken; put() copies at
// once (after open()).  Empty arrays are not copied.
struct ArrayStage : Layout, PendingCopies {
    orbx_ctx* ctx;
    explicit ArrayStage(orbx_ctx* c) : ctx(c) {}
    template <typename T>
    Region<T> take(size_t count, const T* src = nullptr)
    {
        const Region<T> r = Layout::take<T>(count);
        later(r, src);
        return r;
    }
    int open() { return ensure_scratch(ctx, total); }
    int upload()
    {
        const int r = open();
        if (r != ORBX_OK) return r;
        for (const Pending& p : pending)
            ORBX_HIP_CHECK(hipMemcpyAsync(static_cast<uint8_t*>(ctx->scratch) + p.off, p.src, p.bytes,
                                          hipMemcpyHostToDevice, ctx->stream));
        return ORBX_OK;
    }
    template <typename T>
    T* dev(Region<T> r) const
    {
        return region_ptr(ctx->scratch, r);
    }
    template <typename T>
    int put(Region<T> r, const T* src, size_t count)
    {
        if (count && src)
            ORBX_HIP_CHECK(hipMemcpyAsync(dev(r), src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        return ORBX_OK;
    }
    template <typename T>
    int put(Region<T> r, const T* src)
    {
        return put(r, src, r.count);
    }
    template <typename T>
    int fill(Region<T> r, int byte)
    {
        ORBX_HIP_CHECK(hipMemsetAsync(dev(r), byte, r.bytes(), ctx->stream));
        return ORBX_OK;
    }
    template <typename T>
    int get(T* dst, Region<T> r, size_t count)
    {
        if (count) ORBX_HIP_CHECK(hipMemcpyAsync(dst, dev(r), count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        return ORBX_OK;
    }
    template <typename T>
    int get(T* dst, Region<T> r)
    {
        return get(dst, r, r.count);
    }
};

// The packed inputs of a batched solver call on the context stream.
struct PackedStage : PackedLayout {
    orbx_ctx* ctx;
    explicit PackedStage(orbx_ctx* c) : ctx(c) {}
    // in the context scratch, `behind` bytes of result blocks after the inputs
    // (a call that follows a queued search binds to BowQueued::extra instead)
    int open(size_t behind)
    {
        const int r = ensure_scratch(ctx, total + behind);
        if (r == ORBX_OK) bind(ctx->scratch);
        return r;
    }
    uint8_t* behind() const { return base + total; }
    int upload()
    {
        if (total) ORBX_HIP_CHECK(hipMemcpyAsync(base, blob.data(), total, hipMemcpyHostToDevice, ctx->stream));
        return ORBX_OK;
    }
};

// P result blocks of `stride` bytes on the device and their host copy.
struct ResultBlocks {
    orbx_ctx* ctx;
    uint8_t* dev;
    size_t P, stride, pitch = 0;
    std::unique_ptr<uint8_t[]> h;
    ResultBlocks(orbx_ctx* c, uint8_t* d, size_t blocks, size_t s) : ctx(c), dev(d), P(blocks), stride(s) {}
    // for the kernels that count on zeroed blocks
    int zero()
    {
        ORBX_HIP_CHECK(hipMemsetAsync(dev, 0, P * stride, ctx->stream));
        return ORBX_OK;
    }
    // the first `head` bytes of every block (0: all of it), waited for
    int read(size_t head = 0)
    {
        pitch = head ? head : stride;
        h.reset(new (std::nothrow) uint8_t[pitch * P]);
        if (!h) return ORBX_ERR_NOMEM;
        if (pitch == stride)
            ORBX_HIP_CHECK(hipMemcpyAsync(h.get(), dev, P * stride, hipMemcpyDeviceToHost, ctx->stream));
        else
            ORBX_HIP_CHECK(hipMemcpy2DAsync(h.get(), pitch, dev, stride, pitch, P, hipMemcpyDeviceToHost, ctx->stream));
        ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return ORBX_OK;
    }
    const uint8_t* block(size_t k) const { return h.get() + k * pitch; }
};

// Every slot's feature count (ctx->out_n), waited for.
inline int read_slot_counts(orbx_ctx* ctx, std::vector<int32_t>& cnt)
{
    cnt.resize(ctx->slots);
    ORBX_HIP_CHECK(hipMemcpyAsync(cnt.data(), ctx->out_n, sizeof(int32_t) * ctx->slots, hipMemcpyDeviceToHost, ctx->stream));
    ORBX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return ORBX_OK;
}

// Every keypoint's octave indexes a table of nlevels entries.
inline bool octaves_ok(const orbx_keypoint* k, int n, int nlevels)
{
    for (int i = 0; i < n; i++)
        if (k[i].octave < 0 || k[i].octave >= nlevels) return false;
    return true;
}

// ceil(log(1 - p) / log(1 - eps^3)) of both SetRansacParameters (Sim3Solver.cc:114-138, PnPsolver.cc:93-124)
// as the int the device tables hold: a quotient past INT_MAX (or a NaN) saturates, one below 1 is 1.
inline int ransac_iterations(float eps, double probability)
{
    const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)eps, 3)));
    return !(v < 2147483647.0) ? 2147483647 : (v < 1.0 ? 1 : (int)v);
}

}  // namespace orbx
