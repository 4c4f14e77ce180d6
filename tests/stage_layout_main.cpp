// Stand-alone check of orbx_stage.h's layout and host-side copies
// (tests/test_stage_layout.py builds it with ASan + UBSan).  No HIP call.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbx_stage.h"

using namespace orbx;

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("line %d: %s\n", __LINE__, #cond);            \
            failures++;                                               \
        }                                                             \
    } while (0)

struct Span {
    size_t off, bytes;
};

template <typename T>
static Span span(Region<T> r)
{
    return {r.off, r.bytes()};
}

// `what` touched exactly [off, off + bytes) of a buffer pre-filled with 0xA5
// (its own bytes are never 0xA5 here).
static void exact(const std::vector<uint8_t>& buf, size_t off, size_t bytes)
{
    for (size_t i = 0; i < buf.size(); i++) CHECK((buf[i] != 0xA5) == (i >= off && i < off + bytes));
}

int main()
{
    CHECK(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512);

    // sizes around the 256-byte step, empty regions between and at the ends
    Layout l;
    std::vector<Span> s;
    s.push_back(span(l.take<uint8_t>(0)));
    s.push_back(span(l.take<int32_t>(1)));
    s.push_back(span(l.take<int32_t>(1)));
    s.push_back(span(l.take<float>(0)));
    s.push_back(span(l.take<uint8_t>(255)));
    s.push_back(span(l.take<uint8_t>(256)));
    s.push_back(span(l.take<uint8_t>(257)));
    s.push_back(span(l.take<double>(33)));
    s.push_back(span(l.take<orbx_keypoint>(7)));
    s.push_back(span(l.take<int32_t>(0)));
    CHECK(s[0].off == 0);
    CHECK(s[2].off - s[1].off == 256);   // two counters never share a block
    for (size_t i = 0; i < s.size(); i++) {
        CHECK(s[i].off % 256 == 0);
        // the next region starts past this one's last byte and past its
        // first, so an empty region has an address of its own
        const size_t next = i + 1 < s.size() ? s[i + 1].off : l.total;
        CHECK(next >= s[i].off + s[i].bytes);
        CHECK(next > s[i].off);
        CHECK(next - s[i].off == align256(s[i].bytes ? s[i].bytes : 1));
    }
    CHECK(l.total == s.back().off + 256);
    CHECK(l.total % 256 == 0);

    // parts of a region
    const Region<uint8_t> blob{512, 100};
    const Region<int32_t> p = blob.part<int32_t>(20, 5);
    CHECK(p.off == 532 && p.count == 5 && p.bytes() == 20 && p.end() == 552);

    // put / fill / get through a handle, on a host buffer standing in for
    // the pinned block, with guard space on both sides of every region
    BlockStage b(nullptr);
    const Region<uint8_t> guard0 = b.take<uint8_t>(256);
    const Region<int32_t> ints = b.take<int32_t>(5);
    const Region<uint8_t> bytes = b.take<uint8_t>(3);
    const Region<double> dbl = b.take<double>(2);
    const Region<float> none = b.take<float>(0);
    const Region<uint8_t> guard1 = b.take<uint8_t>(256);
    (void)guard0;
    (void)guard1;
    std::vector<uint8_t> buf(b.total);
    b.h = buf.data();
    auto reset = [&] { std::fill(buf.begin(), buf.end(), 0xA5); };

    const int32_t src[5] = {1, 2, 3, 4, 5};
    reset();
    b.put(ints, src);
    exact(buf, ints.off, 20);
    reset();
    b.put(ints, src, 2);   // fewer than reserved
    exact(buf, ints.off, 8);
    reset();
    b.put(ints, static_cast<const int32_t*>(nullptr));   // an absent input
    exact(buf, 0, 0);
    reset();
    b.fill(bytes, 0xFF);
    exact(buf, bytes.off, 3);
    reset();
    b.fill(dbl, 0);
    exact(buf, dbl.off, 16);
    reset();
    b.fill(none, 0);
    b.put(none, static_cast<const float*>(nullptr));
    exact(buf, 0, 0);

    // get writes exactly count * sizeof(T) bytes of the destination
    reset();
    b.put(ints, src);
    std::vector<uint8_t> dst(256 + 20 + 256, 0xA5);
    b.get(reinterpret_cast<int32_t*>(dst.data() + 256), ints);
    exact(dst, 256, 20);
    CHECK(std::memcmp(dst.data() + 256, src, 20) == 0);
    std::fill(dst.begin(), dst.end(), 0xA5);
    b.get(reinterpret_cast<int32_t*>(dst.data() + 256), ints, 3);
    exact(dst, 256, 12);
    std::fill(dst.begin(), dst.end(), 0xA5);
    b.get(static_cast<int32_t*>(nullptr), ints);
    b.get(reinterpret_cast<float*>(dst.data() + 256), none);
    exact(dst, 0, 0);

    // the pointer a handle stands for
    CHECK(reinterpret_cast<uint8_t*>(region_ptr(buf.data(), dbl)) == buf.data() + dbl.off);

    float sc[4];
    level_scales(4, 1.2f, sc);
    CHECK(sc[0] == 1.0f && sc[1] == 1.2f && sc[2] == sc[1] * 1.2f && sc[3] == sc[2] * 1.2f);

    if (failures) std::printf("%d checks failed\n", failures);
    return failures ? 1 : 0;
}
