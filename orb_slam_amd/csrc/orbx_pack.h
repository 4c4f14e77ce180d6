// The offset arithmetic of the staging helpers (orbx_stage.h), free of HIP and
// of the context so that it compiles and is tested on its own
// (tests/pack_check.cpp): Region<T>, the 16-byte block offsets of the solvers'
// result blocks, and the packed layout of a batched solver call's inputs.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace orbx {

inline size_t up16(size_t x) { return (x + 15) & ~size_t(15); }

template <typename T>
struct Region {
    size_t off = 0, count = 0;
    size_t bytes() const { return count * sizeof(T); }
    size_t end() const { return off + bytes(); }
    // n elements of U starting byte_off into this region (rows of an image,
    // one struct of an array, the arrays behind a header)
    template <typename U = T>
    Region<U> part(size_t byte_off, size_t n) const
    {
        return Region<U>{off + byte_off, n};
    }
};

template <typename T>
T* region_ptr(void* base, Region<T> r)
{
    return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + r.off);
}

// Byte offsets inside one result block: every array on a 16-byte boundary,
// `end` the block's stride once all are taken.
struct BlockOffsets {
    long long end = 0;
    long long take(long long bytes)
    {
        const long long r = end;
        end += (bytes + 15) & ~15ll;
        return r;
    }
};

// The sources a stage copies to their regions once the layout is complete.
struct PendingCopies {
    struct Pending {
        size_t off;
        const void* src;
        size_t bytes;
    };
    std::vector<Pending> pending;
    // also for a source known after its region was taken, or shorter than it (part())
    template <typename T>
    void later(Region<T> r, const T* src)
    {
        if (src && r.count) pending.push_back({r.off, src, r.bytes()});
    }
};

// The inputs of one batched call, packed at 16-byte granularity into one host
// blob that mirrors its device range offset for offset.  take() is the only
// statement of an array's size; it is called while the arguments are checked,
// so `total` is known before there is a device address.  bind() then fixes
// the device base, allocates the zero-filled blob (padding stays zero) and
// copies every source named at take() or later() to its offset.  An empty
// region may share its address with the next one.
struct PackedLayout : PendingCopies {
    size_t total = 0;
    std::vector<uint8_t> blob;
    uint8_t* base = nullptr;

    template <typename T>
    Region<T> take(size_t count, const T* src = nullptr)
    {
        const Region<T> r{total, count};
        total += up16(r.bytes());
        later(r, src);
        return r;
    }
    void align_end(size_t a) { total = (total + a - 1) / a * a; }
    void bind(void* device_base)
    {
        base = static_cast<uint8_t*>(device_base);
        blob.assign(total, 0);
        for (const Pending& p : pending) std::memcpy(blob.data() + p.off, p.src, p.bytes);
    }
    // arrays that are computed rather than copied are written here (after bind)
    template <typename T>
    T* host(Region<T> r)
    {
        return region_ptr(blob.data(), r);
    }
    template <typename T>
    T* dev(Region<T> r) const
    {
        return region_ptr(base, r);
    }
};

}  // namespace orbx
