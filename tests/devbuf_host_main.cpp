// Stand-alone check of style_transfer2_amd/csrc/devbuf.h on the host (tests/test_devbuf_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it).  The two funnel pairs sit over malloc / free here, with the live-byte counters of
// the engine's funnel and a switch that fails the N-th allocation.  Exit status 0: every property below holds.
#include "../style_transfer2_amd/csrc/devbuf.h"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

static long long g_dev = 0, g_pin = 0, g_dev_peak = 0, g_frees = 0;
static int g_fail_at = 0;          // > 0: the g_fail_at-th allocation from now fails

namespace st2e {
static int host_alloc(void** p, size_t bytes, long long& live)
{
    if (g_fail_at > 0 && --g_fail_at == 0) return ST_ERR_HIP;
    void* q = malloc(bytes);
    if (!q) return ST_ERR_HIP;
    live += (long long)bytes;
    g_dev_peak = std::max(g_dev_peak, g_dev);
    *p = q;
    return ST_OK;
}
int raw_alloc(void** p, size_t bytes) { return host_alloc(p, bytes, g_dev); }
void raw_free(void* p, size_t bytes) { free(p); g_dev -= (long long)bytes; ++g_frees; }
int raw_pin_alloc(void** p, size_t bytes) { return host_alloc(p, bytes, g_pin); }
void raw_pin_free(void* p, size_t bytes) { free(p); g_pin -= (long long)bytes; ++g_frees; }
}  // namespace st2e
using namespace st2e;

static int g_bad = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_bad; } \
    } while (0)

int main()
{
    const long long F = sizeof(float);
    {   // a default-constructed buffer is empty; a moved-from buffer is empty and its block is freed once
        DevBuf<float> a;
        CHECK(!a && a.get() == nullptr && a.cap() == 0);
        CHECK(a.alloc(10) == ST_OK && a && a.cap() == 10 && g_dev == 10 * F);
        a[9] = 1.f;                                   // the whole block is ours (ASan would object)
        float* was = a;
        const long long frees = g_frees;
        DevBuf<float> b(std::move(a));
        CHECK(!a && a.get() == nullptr && a.cap() == 0 && b.get() == was && b.cap() == 10 && g_dev == 10 * F);
        DevBuf<float> c;
        CHECK(c.alloc(3) == ST_OK && g_dev == 13 * F);
        c = std::move(b);                             // the target's own block goes, the source's is taken over
        CHECK(!b && b.cap() == 0 && c.get() == was && c.cap() == 10 && g_dev == 10 * F && g_frees == frees + 1);
        DevBuf<float>& same = c;
        c = std::move(same);                          // self-move keeps the block
        CHECK(c.get() == was && g_dev == 10 * F);
        a.reset(); b.reset();                         // nothing to free
        CHECK(g_frees == frees + 1);
        c.reset();
        CHECK(!c && g_dev == 0 && g_frees == frees + 2);
        c.reset();
        CHECK(g_frees == frees + 2);
    }
    CHECK(g_dev == 0 && g_pin == 0);
    {   // reserve: grow-only, keeps the pointer when there is room, frees BEFORE it allocates when there is not
        DevBuf<float> a;
        CHECK(a.reserve(100) == ST_OK && a.cap() == 100);
        float* was = a;
        CHECK(a.reserve(100) == ST_OK && a.reserve(7) == ST_OK && a.reserve(0) == ST_OK && a.get() == was && a.cap() == 100);
        g_dev_peak = g_dev;
        CHECK(a.reserve(150) == ST_OK && a.cap() == 150 && g_dev == 150 * F && g_dev_peak == 150 * F);      // never 250
        a[149] = 2.f;
        // alloc: exactly n, also downwards
        g_dev_peak = g_dev;
        CHECK(a.alloc(20) == ST_OK && a.cap() == 20 && g_dev == 20 * F && g_dev_peak == 150 * F);
    }
    CHECK(g_dev == 0);
    {   // a failed reserve / alloc leaves an empty buffer, and the counter without the old block
        DevBuf<float> a;
        CHECK(a.alloc(50) == ST_OK);
        g_fail_at = 1;
        CHECK(a.reserve(60) == ST_ERR_HIP && a.get() == nullptr && a.cap() == 0 && !a && g_dev == 0);
        CHECK(a.alloc(50) == ST_OK && g_dev == 50 * F);
        g_fail_at = 1;
        CHECK(a.alloc(50) == ST_ERR_HIP && a.get() == nullptr && a.cap() == 0 && g_dev == 0);
        CHECK(a.reserve(5) == ST_OK && a.cap() == 5);             // ... and is usable again
    }
    CHECK(g_dev == 0);
    {   // minimum sizes: 1 float, 8 bf16 (kernels read whole vectors at the tail); the pinned sibling counts on its own
        DevBuf<float> f;
        DevBuf<unsigned short> h;
        CHECK(f.alloc(0) == ST_OK && f && f.cap() == 0 && g_dev == F);
        f[0] = 3.f;
        CHECK(h.alloc(3) == ST_OK && h.cap() == 3 && g_dev == F + 8 * 2);
        h[7] = 1;
        CHECK(h.alloc(9) == ST_OK && g_dev == F + 9 * 2);
        f.reset(); h.reset();
        CHECK(g_dev == 0);
        DevBuf<double> d;
        DevBuf<unsigned char> u;
        CHECK(d.alloc(3) == ST_OK && u.alloc(5) == ST_OK && g_dev == 3 * 8 + 5);
        PinBuf<char> p;
        CHECK(p.alloc(4096 + 12) == ST_OK && g_pin == 4096 + 12 && g_dev == 3 * 8 + 5);
        char* img = p + 4096;
        img[11] = 1;
        PinBuf<char> q(std::move(p));
        CHECK(!p && g_pin == 4096 + 12);
    }
    CHECK(g_dev == 0 && g_pin == 0);
    {   // a vector of buffers that is resized, reassigned and destroyed
        std::vector<DevBuf<float>> v(4);
        for (size_t i = 0; i < v.size(); ++i) CHECK(v[i].alloc(10 * (i + 1)) == ST_OK);
        CHECK(g_dev == 100 * F);
        v.resize(64);                                 // reallocates: the elements move
        CHECK(g_dev == 100 * F && v[3].cap() == 40 && !v[4]);
        v[2][29] = 4.f;
        v.resize(2);
        CHECK(g_dev == 30 * F);
        v.erase(v.begin());                           // (Pipe::retired erases from the middle)
        CHECK(g_dev == 20 * F && v[0].cap() == 20);
        std::vector<DevBuf<float>> w(3);
        CHECK(w[1].alloc(5) == ST_OK && g_dev == 25 * F);
        v = std::move(w);
        CHECK(g_dev == 5 * F && v.size() == 3 && v[1].cap() == 5);
        v = std::vector<DevBuf<float>>(2);
        CHECK(g_dev == 0);
        std::vector<PinBuf<float>> pv(3);
        CHECK(pv[0].alloc(6) == ST_OK && g_pin == 6 * F);
    }
    CHECK(g_dev == 0 && g_pin == 0);
    {   // a scope with five buffers whose third allocation fails (the shape of every ST_TRY chain in the engine)
        auto chain = []() -> int {
            DevBuf<float> b[5];
            for (int i = 0; i < 5; ++i) {
                const int rc = b[i].alloc(16);
                if (rc != ST_OK) return rc;
            }
            return ST_OK;
        };
        g_fail_at = 3;
        CHECK(chain() == ST_ERR_HIP);
        CHECK(g_dev == 0);
        g_fail_at = 0;
        CHECK(chain() == ST_OK);
    }
    CHECK(g_dev == 0 && g_pin == 0);
    if (g_bad) { printf("%d check(s) failed\n", g_bad); return 1; }
    printf("devbuf: all checks passed\n");
    return 0;
}
