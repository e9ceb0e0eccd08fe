// Host driver for tests/test_lightmap_unwrap_cpu.py: include/lupin_pack.hpp -- the shelf packer, the rectangle arithmetic and
// the descriptor checks of lupin_hip_unwrap_lightmap_uvs -- in a stand-alone program built with -fsanitize=address,undefined.
// Nothing is loaded into Python.  It walks the packer over the cases the tests name (one rectangle, equal rectangles, a
// rectangle as wide as the atlas, none at all, many of mixed sizes, the largest sides) and checks what it returns itself:
// no two rectangles intersect, all lie inside width x height.  Exit status 0: every check held.
#include <cmath>
#include <cstdio>
#include <limits>

#include "lupin_pack.hpp"

using lupin_pack::Rect;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static void pack_and_check(std::vector<Rect> rects, uint64_t want_width = 0)
{
    const std::vector<Rect> before = rects;
    uint64_t W = 0, H = 0;
    lupin_pack::shelf_pack(rects, &W, &H);
    CHECK(rects.size() == before.size());
    if (want_width) CHECK(W == want_width);
    uint64_t area = 0;
    for (size_t i = 0; i < rects.size(); i++)
    {
        const Rect &a = rects[i];
        area += (uint64_t)a.w * a.h;
        CHECK((uint64_t)a.x + a.w <= W && (uint64_t)a.y + a.h <= H);
        CHECK(a.w == before[a.label].w && a.h == before[a.label].h);      // labels are indices here: nothing was mixed up
        if (i > 0)
        {
            const Rect &p = rects[i - 1];
            CHECK(p.h > a.h || (p.h == a.h && (p.w > a.w || (p.w == a.w && p.label < a.label))));
        }
        for (size_t j = 0; j < i; j++)
        {
            const Rect &b = rects[j];
            const bool apart = a.x + a.w <= b.x || b.x + b.w <= a.x || a.y + a.h <= b.y || b.y + b.h <= a.y;
            CHECK(apart);
        }
    }
    CHECK(W * W >= area || rects.empty() || W >= 1);
    CHECK(W * H >= area);
}

int main()
{
    using lupin_pack::isqrt_ceil;
    CHECK(isqrt_ceil(0) == 0 && isqrt_ceil(1) == 1 && isqrt_ceil(2) == 2 && isqrt_ceil(4) == 2 && isqrt_ceil(5) == 3);
    CHECK(isqrt_ceil((1ull << 32) * (1ull << 30)) == (1ull << 31));
    CHECK(isqrt_ceil(16384ull * 16384ull) == 16384 && isqrt_ceil(16384ull * 16384ull + 1) == 16385);
    for (uint64_t n = 0; n < 5000; n++)
    {
        const uint64_t r = isqrt_ceil(n);
        CHECK(r * r >= n && (r == 0 || (r - 1) * (r - 1) < n));
    }

    pack_and_check({});
    pack_and_check({Rect{7, 3, 0, 0, 0}}, 7);                                        // one rectangle: the atlas is the rectangle
    pack_and_check({Rect{4, 4, 0, 0, 0}, Rect{4, 4, 1, 0, 0}, Rect{4, 4, 2, 0, 0}, Rect{4, 4, 3, 0, 0}}, 8);   // equal rectangles
    pack_and_check({Rect{40, 2, 0, 0, 0}, Rect{3, 5, 1, 0, 0}, Rect{3, 3, 2, 0, 0}}, 40);      // one as wide as the atlas
    pack_and_check({Rect{16384, 16384, 0, 0, 0}, Rect{16384, 1, 1, 0, 0}});
    {
        std::vector<Rect> many;
        uint32_t s = 12345u;
        for (uint32_t i = 0; i < 700; i++)
        {
            s = s * 1664525u + 1013904223u;
            many.push_back(Rect{1u + (s >> 8) % 37u, 1u + (s >> 16) % 23u, i, 0, 0});
        }
        pack_and_check(many);
    }

    // the descriptor checks
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(lupin_pack::unwrap_desc_refusal(0.01f, 0, 0) == nullptr && lupin_pack::unwrap_desc_refusal(1e30f, 16, 0) == nullptr);
    CHECK(lupin_pack::unwrap_desc_refusal(0.0f, 0, 0) && lupin_pack::unwrap_desc_refusal(-1.0f, 0, 0) && lupin_pack::unwrap_desc_refusal(inf, 0, 0));
    CHECK(lupin_pack::unwrap_desc_refusal(nan, 0, 0) && lupin_pack::unwrap_desc_refusal(1.0f, 17, 0) && lupin_pack::unwrap_desc_refusal(1.0f, 0, 1));
    CHECK(lupin_pack::unwrap_desc_refusal(1.0f, 0xFFFFFFFFu, 0) && lupin_pack::unwrap_desc_refusal(1.0f, 0, 0x80000000u));

    // the rectangle arithmetic: no float ever reaches an integer conversion it does not fit
    uint32_t e = 99;
    CHECK(lupin_pack::extent_texels(0.0f, 0.0f, 1.0f, &e) && e == 1);
    CHECK(lupin_pack::extent_texels(-1.0f, 1.5f, 0.5f, &e) && e == 5);
    CHECK(lupin_pack::extent_texels(0.0f, 16384.0f, 1.0f, &e) && e == 16384);
    e = 99;
    CHECK(!lupin_pack::extent_texels(0.0f, 16384.5f, 1.0f, &e) && e == 99);
    CHECK(!lupin_pack::extent_texels(-3e38f, 3e38f, 1.0f, &e) && !lupin_pack::extent_texels(0.0f, 1.0f, 1e-30f, &e) && e == 99);
    CHECK(!lupin_pack::extent_texels(nan, 1.0f, 1.0f, &e) && !lupin_pack::extent_texels(0.0f, inf, 1.0f, &e) && e == 99);
    CHECK(lupin_pack::instance_side(10, 1.5f, 2, &e) && e == 19);
    CHECK(lupin_pack::instance_side(1, 1e-20f, 0, &e) && e == 1);
    e = 99;
    CHECK(!lupin_pack::instance_side(0, 1.0f, 0, &e) && !lupin_pack::instance_side(8, 0.0f, 0, &e) && !lupin_pack::instance_side(8, nan, 0, &e));
    CHECK(!lupin_pack::instance_side(8, inf, 0, &e) && !lupin_pack::instance_side(16384, 1.0f, 1, &e) && !lupin_pack::instance_side(8, 1e30f, 0, &e));
    CHECK(!lupin_pack::instance_side(8, 1.0f, 0xFFFFFFFFu, &e) && !lupin_pack::instance_side(0xFFFFFFFFu, 1.0f, 0, &e) && e == 99);

    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("lupin_pack: every check held\n");
    return 0;
}
