// include/lupin_stitch_rules.hpp on the host alone, built with -fsanitize=address,undefined by
// tests/test_lightmap_stitch_cpu.py: the descriptor's refusals in the order the library looks, the sort bits and the count
// limits at their edges.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "lupin_stitch_rules.hpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static bool says(const char *got, const char *want) { return got && std::strstr(got, want) != nullptr; }

int main()
{
    using namespace lupin_stitch;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(desc_refusal(1, 1, 0, 2.0f, 0.1f, 0, 0) == nullptr);
    CHECK(desc_refusal(MAX_SIZE, MAX_SIZE, MAX_ITERATIONS, 1e-30f, 1e30f, DEVICE_POINTERS, 0) == nullptr);
    CHECK(says(desc_refusal(0, 1, 0, 2.0f, 0.1f, 0, 0), "width"));
    CHECK(says(desc_refusal(1, 0, 0, 2.0f, 0.1f, 0, 0), "width"));
    CHECK(says(desc_refusal(MAX_SIZE + 1, 1, 0, 2.0f, 0.1f, 0, 0), "width"));
    CHECK(says(desc_refusal(1, MAX_SIZE + 1, 0, 2.0f, 0.1f, 0, 0), "width"));
    CHECK(says(desc_refusal(1, 1, MAX_ITERATIONS + 1, 2.0f, 0.1f, 0, 0), "iterations"));
    CHECK(says(desc_refusal(1, 1, 0xFFFFFFFFu, 2.0f, 0.1f, 0, 0), "iterations"));
    for (float bad : {0.0f, -0.0f, -1.0f, inf, -inf, nan})
    {
        CHECK(says(desc_refusal(1, 1, 1, bad, 0.1f, 0, 0), "samples_per_texel"));
        CHECK(says(desc_refusal(1, 1, 1, 2.0f, bad, 0, 0), "lambda"));
    }
    CHECK(says(desc_refusal(1, 1, 1, 2.0f, 0.1f, 2, 0), "flag"));
    CHECK(says(desc_refusal(1, 1, 1, 2.0f, 0.1f, 3, 0), "flag"));
    CHECK(says(desc_refusal(1, 1, 1, 2.0f, 0.1f, 0x80000000u, 0), "flag"));
    CHECK(says(desc_refusal(1, 1, 1, 2.0f, 0.1f, 0, 1), "reserved"));
    // the first refusal in the order of the checks decides
    CHECK(says(desc_refusal(0, 1, MAX_ITERATIONS + 1, nan, nan, 2, 1), "width"));
    CHECK(says(desc_refusal(1, 1, MAX_ITERATIONS + 1, nan, nan, 2, 1), "iterations"));
    CHECK(says(desc_refusal(1, 1, 1, 2.0f, nan, 2, 1), "lambda"));

    CHECK(bits_for(0) == 1 && bits_for(1) == 1 && bits_for(2) == 2 && bits_for(3) == 2 && bits_for(4) == 3);
    CHECK(bits_for(0xFFFFFFFFull) == 32 && bits_for(0x100000000ull) == 33 && bits_for(~0ull) == 64);
    CHECK(bits_for(16384ull * 16384ull) == 29);
    for (uint64_t v : {1ull, 5ull, 255ull, 256ull, 65535ull, 1ull << 28})
        CHECK((v >> bits_for(v)) == 0 && (bits_for(v) == 1 || (v >> (bits_for(v) - 1)) == 1));

    CHECK(half_edges_ok(0) && half_edges_ok(1431655764ull) && !half_edges_ok(1431655765ull));      // 3 * 1431655764 = 2^32 - 4
    CHECK(pairs_ok(0) && pairs_ok(536870911ull) && !pairs_ok(536870912ull));                       // 8 * 536870911 = 2^32 - 8
    CHECK(!half_edges_ok(~0ull) && !pairs_ok(~0ull));
    std::printf(failures ? "%d checks failed\n" : "stitch rules OK\n", failures);
    return failures ? 1 : 0;
}
