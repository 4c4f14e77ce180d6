// Stand-alone check of orbx_pack.h, the packed layout of the batched solver
// calls' inputs (tests/test_pack_layout.py builds it with ASan + UBSan).
// Standard headers and the C ABI's structs only: no HIP, no context.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "orbx.h"
#include "orbx_pack.h"

using namespace orbx;

static int failures = 0;
#define CHECK(cond)                                        \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("line %d: %s\n", __LINE__, #cond); \
            failures++;                                    \
        }                                                  \
    } while (0)

struct E12 {
    uint8_t b[12];
};
struct E16 {
    uint8_t b[16];
};
static_assert(sizeof(E12) == 12 && sizeof(E16) == 16, "element sizes");

constexpr int kTypes = 6, kCounts = 5;
static const size_t kElem[kTypes] = {1, 4, 8, 12, 16, sizeof(orbx_keypoint)};
static const size_t kCount[kCounts] = {0, 1, 15, 16, 17};

struct Entry {
    int type;
    size_t count, off = 0;
    std::vector<uint8_t> src;   // empty: no source
    bool null_src = false;
    size_t bytes() const { return count * kElem[type]; }
};

// f.template operator()<T>() for the entry's element type
template <typename F>
static auto by_type(int type, F f)
{
    switch (type) {
    case 0: return f(static_cast<uint8_t*>(nullptr));
    case 1: return f(static_cast<int32_t*>(nullptr));
    case 2: return f(static_cast<double*>(nullptr));
    case 3: return f(static_cast<E12*>(nullptr));
    case 4: return f(static_cast<E16*>(nullptr));
    default: return f(static_cast<orbx_keypoint*>(nullptr));
    }
}

static size_t round16(size_t b) { return (b + 15) / 16 * 16; }

// All 30 (element size, count) pairs in the order `perm` gives, every fourth
// one without a source.
static void run(const std::vector<int>& perm)
{
    std::vector<Entry> es;
    for (size_t i = 0; i < perm.size(); i++) {
        Entry e;
        e.type = perm[i] / kCounts;
        e.count = kCount[perm[i] % kCounts];
        e.null_src = i % 4 == 3;
        // a non-null source even where the region is empty (never read then)
        e.src.assign(e.bytes() + 1, 0);
        for (size_t k = 0; k < e.src.size(); k++) e.src[k] = (uint8_t)(1 + (i * 31 + k) % 255);
        es.push_back(e);
    }
    PackedLayout pl;
    size_t expect_off = 0;
    for (Entry& e : es) {
        e.off = by_type(e.type, [&](auto* tag) {
            using T = std::remove_pointer_t<decltype(tag)>;
            const T* src = e.null_src ? nullptr : reinterpret_cast<const T*>(e.src.data());
            const Region<T> r = pl.take<T>(e.count, src);
            CHECK(r.count == e.count && r.bytes() == e.bytes());
            return r.off;
        });
        CHECK(e.off % 16 == 0);
        CHECK(e.off == expect_off);   // take order, no overlap, no gap beyond the rounding
        expect_off += round16(e.bytes());
        CHECK(pl.total == expect_off);   // the sum of the rounded sizes, before any base is known
    }
    for (size_t i = 0; i + 1 < es.size(); i++) CHECK(es[i].off + es[i].bytes() <= es[i + 1].off);

    // what the blob must hold: zeros, and each source at its offset
    std::vector<uint8_t> want(pl.total, 0);
    for (const Entry& e : es)
        if (!e.null_src && e.bytes()) std::memcpy(want.data() + e.off, e.src.data(), e.bytes());

    std::vector<uint8_t> dev_a(pl.total + 1), dev_b(pl.total + 1);
    for (uint8_t* base : {dev_a.data(), dev_b.data()}) {
        pl.bind(base);
        CHECK(pl.blob.size() == pl.total);
        CHECK(pl.blob == want);   // byte for byte at its offset, every other byte still zero
        for (const Entry& e : es)
            by_type(e.type, [&](auto* tag) {
                using T = std::remove_pointer_t<decltype(tag)>;
                const Region<T> r{e.off, e.count};
                CHECK(reinterpret_cast<uint8_t*>(pl.dev(r)) == base + e.off);
                CHECK(reinterpret_cast<uint8_t*>(pl.host(r)) == pl.blob.data() + e.off);
                return 0;
            });
    }
}

int main()
{
    CHECK(up16(0) == 0 && up16(1) == 16 && up16(16) == 16 && up16(17) == 32);

    const int n = kTypes * kCounts;
    std::vector<int> fwd(n), rev(n), by_count(n), mixed(n);
    for (int i = 0; i < n; i++) {
        fwd[i] = i;
        rev[i] = n - 1 - i;
        by_count[i] = (i % kTypes) * kCounts + i / kTypes;   // counts outermost
        mixed[i] = i * 7 % n;                                // 7 and 30 are coprime
    }
    run(fwd);
    run(rev);
    run(by_count);
    run(mixed);

    // empty regions with a null source, alone and between others: accepted,
    // nothing pending, the address shared with what follows
    {
        PackedLayout pl;
        const Region<float> none0 = pl.take<float>(0);
        const Region<int32_t> a = pl.take<int32_t>(17);
        const Region<orbx_keypoint> none1 = pl.take<orbx_keypoint>(0, nullptr);
        const Region<uint8_t> b = pl.take<uint8_t>(31);
        const Region<double> none2 = pl.take<double>(0);
        CHECK(none0.off == 0 && a.off == 0 && none1.off == 80 && b.off == 80 && none2.off == 112 && pl.total == 112);
        CHECK(pl.pending.empty());
        // a source named later, shorter than its region
        const uint8_t five[5] = {9, 8, 7, 6, 5};
        pl.later(b.part(0, 5), five);
        pl.later(none2, static_cast<const double*>(nullptr));
        CHECK(pl.pending.size() == 1);
        pl.align_end(256);
        CHECK(pl.total == 256);
        std::vector<uint8_t> dev(pl.total);
        pl.bind(dev.data());
        std::vector<uint8_t> want(256, 0);
        std::memcpy(want.data() + 80, five, 5);
        CHECK(pl.blob == want);
        pl.host(a)[16] = 0x01020304;   // a computed array is written through host()
        CHECK(std::memcmp(pl.blob.data() + 64, pl.host(a) + 16, 4) == 0);
        CHECK(reinterpret_cast<uint8_t*>(pl.dev(none2)) == dev.data() + 112);
    }
    {
        PackedLayout pl;   // nothing taken
        pl.bind(nullptr);
        CHECK(pl.total == 0 && pl.blob.empty());
    }

    // the result blocks' offsets: the same 16-byte step
    BlockOffsets o;
    CHECK(o.take(100) == 0 && o.take(0) == 112 && o.take(1) == 112 && o.take(16) == 128 && o.end == 144);

    if (failures) std::printf("%d checks failed\n", failures);
    return failures ? 1 : 0;
}
