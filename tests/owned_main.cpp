// Stand-alone host program for tests/test_owned_cpu.py: the owner template and grow_buffer of csrc/lupin_owned.hpp over a
// counting allocator (malloc / free, a set of live pointers, a switch that fails the next allocation), built with
// -fsanitize=address,undefined.  Exit status 0 = every check held and nothing is live at the end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>

#include "../lupinpathtracer_amd/csrc/lupin_owned.hpp"

static std::set<void *> g_live;
static bool g_fail_next = false;
static int g_frees = 0;

struct CountingApi
{
    using Error = int;
    static constexpr int success = 0;
    static int alloc(void **p, size_t bytes)
    {
        if (g_fail_next) { g_fail_next = false; return 2; }   // *p untouched, as hipMalloc leaves it on failure
        void *q = malloc(bytes ? bytes : 1);
        if (!q) return 2;
        memset(q, 0xA5, bytes);   // the sanitizer checks the block is really `bytes` long
        g_live.insert(q);
        *p = q;
        return 0;
    }
    static void free(void *p)
    {
        if (!g_live.erase(p)) { fprintf(stderr, "free of a pointer that is not live: %p\n", p); abort(); }
        g_frees++;
        ::free(p);
    }
};
using Buf = Owned<CountingApi>;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

static int run()
{
    {   // make; a failed make into an empty owner leaves it empty
        Buf a;
        CHECK(a.get() == nullptr);
        g_fail_next = true;
        CHECK(Buf::make(64, &a) != 0 && a.get() == nullptr && g_live.empty());
        CHECK(Buf::make(64, &a) == 0 && a.get() != nullptr && g_live.count(a.get()) == 1 && g_live.size() == 1);
        a.as<unsigned char>()[63] = 1;
        // a failed make into a full owner leaves its old pointer alive and unchanged
        void *old = a.get();
        g_fail_next = true;
        CHECK(Buf::make(128, &a) != 0 && a.get() == old && g_live.count(old) == 1 && g_live.size() == 1);
        // a successful make into a full owner frees the old block
        const int frees = g_frees;
        CHECK(Buf::make(128, &a) == 0 && a.get() != nullptr && g_live.size() == 1 && g_live.count(a.get()) == 1 && g_frees == frees + 1);
    }
    CHECK(g_live.empty());
    {   // move construction
        Buf a;
        CHECK(Buf::make(32, &a) == 0);
        void *p = a.get();
        Buf b(std::move(a));
        CHECK(a.get() == nullptr && b.get() == p && g_live.size() == 1);
    }
    CHECK(g_live.empty());
    {   // move assignment onto a full owner frees the old block exactly once
        Buf a, b;
        CHECK(Buf::make(32, &a) == 0 && Buf::make(48, &b) == 0);
        void *pa = a.get(), *pb = b.get();
        const int frees = g_frees;
        b = std::move(a);
        CHECK(a.get() == nullptr && b.get() == pa && g_live.count(pb) == 0 && g_live.count(pa) == 1 && g_frees == frees + 1);
        // self-move-assignment is harmless
        Buf &alias = b;
        b = std::move(alias);
        CHECK(b.get() == pa && g_live.count(pa) == 1 && g_frees == frees + 1);
    }
    CHECK(g_live.empty());
    {   // reset() then make(); reset() of an empty owner
        Buf a;
        a.reset();
        CHECK(Buf::make(16, &a) == 0);
        const int frees = g_frees;
        a.reset();
        CHECK(a.get() == nullptr && g_live.empty() && g_frees == frees + 1);
        a.reset();
        CHECK(g_frees == frees + 1);
        CHECK(Buf::make(24, &a) == 0 && a.get() != nullptr && g_live.size() == 1);
    }
    CHECK(g_live.empty());
    {   // swap: full with full, full with empty
        Buf a, b, c;
        CHECK(Buf::make(8, &a) == 0 && Buf::make(8, &b) == 0);
        void *pa = a.get(), *pb = b.get();
        const int frees = g_frees;
        a.swap(b);
        CHECK(a.get() == pb && b.get() == pa);
        a.swap(c);
        CHECK(a.get() == nullptr && c.get() == pb && g_frees == frees && g_live.size() == 2);
    }
    CHECK(g_live.empty());
    {   // the shape of ensure_path_buffers: nine owners, all freed first, the sixth make fails
        Buf nine[9];
        for (Buf &b : nine) CHECK(Buf::make(100, &b) == 0);
        CHECK(g_live.size() == 9);
        for (Buf &b : nine) b.reset();
        CHECK(g_live.empty());
        int made = 0;
        for (int k = 0; k < 9; k++)
        {
            if (k == 5) g_fail_next = true;
            if (Buf::make(200, &nine[k]) != 0) break;
            made++;
        }
        CHECK(made == 5 && g_live.size() == 5);
        for (int k = 0; k < 9; k++) CHECK((nine[k].get() != nullptr) == (k < 5));
    }
    CHECK(g_live.empty());
    {   // grow_buffer: smaller keeps, larger replaces, a failed larger request keeps the old block and its size
        Buf a;
        size_t have = 0;
        CHECK(grow_buffer(&a, &have, 100) == 0 && have == 100 && a.get() != nullptr);
        void *p = a.get();
        CHECK(grow_buffer(&a, &have, 40) == 0 && have == 100 && a.get() == p);
        CHECK(grow_buffer(&a, &have, 100) == 0 && have == 100 && a.get() == p);
        g_fail_next = true;
        CHECK(grow_buffer(&a, &have, 300) != 0 && have == 100 && a.get() == p && g_live.count(p) == 1 && g_live.size() == 1);
        CHECK(grow_buffer(&a, &have, 300) == 0 && have == 300 && g_live.count(p) == 0 && g_live.size() == 1 && g_live.count(a.get()) == 1);
        a.as<unsigned char>()[299] = 1;
    }
    CHECK(g_live.empty());
    return 0;
}

int main()
{
    const int rc = run();
    if (rc == 0 && !g_live.empty()) { fprintf(stderr, "%zu blocks live at exit\n", g_live.size()); return 1; }
    if (rc == 0) printf("owned OK (%d frees)\n", g_frees);
    return rc;
}
