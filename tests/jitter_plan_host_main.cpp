// csrc/jitter_plan.h on the host, alone (no HIP, no engine), under the address and undefined-behaviour sanitizers
// (tests/test_jitter_plan_cpu.py builds and runs it).  Lines:
//   validate <radius> -> <refusal text>
//   draw <seed> <k> -> <r_k>
//   shift <seed> <R> <k> -> <dy> <dx>
//   reduce <d> <n> -> <reduced>
//   roll <H> <W> <dy> <dx> -> <rdy> <rdx> <form> <once> <sum>     per form the launcher can take (0 scalar, 1 16-byte): once: 1 when the walk
//        of roll_k over the planned grid writes every element of a destination of exactly 3 H W floats once and reads every source
//        element once; sum: sum over i of dst[i] * (i + 1) mod 2^64 for the source 0, 1, 2, ...
//   plan_refused / big <rows> <gx> <gy> <gx_vec> <gy_vec>
#include "../style_transfer2_amd/csrc/jitter_plan.h"

#include <limits.h>
#include <stdio.h>
#include <vector>

using namespace st2;

// the walk of roll_k<VEC>: workgroup (bx, by), thread (tx, ty); sources through jitter_src, like the kernel
static void walk(const JitterPlan& p, bool vec, std::vector<uint32_t>& dst, std::vector<unsigned char>& wrote, std::vector<unsigned char>& read,
                 const std::vector<uint32_t>& src)
{
    const int PX = vec ? 4 : 1;
    const unsigned gx = vec ? p.gx_vec : p.gx, gy = vec ? p.gy_vec : p.gy;
    for (unsigned by = 0; by < gy; ++by)
        for (unsigned bx = 0; bx < gx; ++bx)
            for (int ty = 0; ty < kJitBlockY; ++ty)
                for (int tx = 0; tx < kJitBlockX; ++tx) {
                    const int x0 = (int)(bx * kJitBlockX + tx) * PX;
                    if (x0 >= p.W) continue;
                    int sx[4];
                    sx[0] = jitter_src(x0, p.dx, p.W);
                    for (int j = 1; j < PX; ++j) sx[j] = sx[j - 1] + 1 == p.W ? 0 : sx[j - 1] + 1;
                    for (long long row0 = (long long)by * kJitTripRows + ty; row0 < p.rows; row0 += (long long)gy * kJitTripRows)
                        for (int r = 0; r < kJitRows; ++r) {
                            const long long row = row0 + r * kJitBlockY;
                            if (row >= p.rows) continue;
                            const int ch = (int)(row / p.H), y = (int)(row - (long long)ch * p.H);
                            const size_t s = ((size_t)ch * p.H + jitter_src(y, p.dy, p.H)) * p.W;
                            for (int j = 0; j < PX; ++j) {
                                dst.at((size_t)row * p.W + x0 + j) = src.at(s + sx[j]);
                                wrote.at((size_t)row * p.W + x0 + j) += 1;
                                read.at(s + sx[j]) += 1;
                            }
                        }
                }
}

static int roll_case(int H, int W, int dy, int dx, unsigned force_gy = 0)
{
    JitterPlan p;
    if (jitter_plan(H, W, dy, dx, &p) != JITTER_OK || p.H != H || p.W != W || p.rows != 3 * H || p.pixels != (size_t)3 * H * W) return 1;
    if (p.dy < 0 || p.dy >= H || p.dx < 0 || p.dx >= W || p.row_vec != (W % 4 == 0)) return 1;
    if (force_gy) p.gy = p.gy_vec = force_gy;              // (the kernel strides by the grid it is given: fewer workgroups, more trips)
    std::vector<uint32_t> src(p.pixels);
    for (size_t i = 0; i < p.pixels; ++i) src[i] = (uint32_t)i;
    for (int form = 0; form < (p.row_vec ? 2 : 1); ++form) {
        std::vector<uint32_t> dst(p.pixels, 0xFFFFFFFFu);   // exactly the planes' size
        std::vector<unsigned char> wrote(p.pixels, 0), read(p.pixels, 0);
        walk(p, form == 1, dst, wrote, read, src);
        int once = 1;
        uint64_t sum = 0;
        for (size_t i = 0; i < p.pixels; ++i) {
            if (wrote[i] != 1 || read[i] != 1) once = 0;
            sum += (uint64_t)dst[i] * (uint64_t)(i + 1);
        }
        printf("roll %d %d %d %d -> %d %d %d %d %llu\n", H, W, dy, dx, p.dy, p.dx, form, once, (unsigned long long)sum);
    }
    return 0;
}

int main()
{
    const int radii[] = {INT_MIN, -1, 0, 1, 3, 4096, 4097, INT_MAX};
    for (int r : radii) printf("validate %d -> %s\n", r, jitter_refusal_text(jitter_validate_radius(r)));

    for (uint64_t k = 0; k < 3; ++k) printf("draw %llu %llu -> %llu\n", 1234567ull, (unsigned long long)k, (unsigned long long)jitter_draw(1234567ull, k));
    const uint64_t seeds[] = {0ull, 7ull, 0xFFFFFFFFFFFFFFFFull};
    const int rs[] = {1, 3, 16, 1024, 4096};
    for (uint64_t seed : seeds)
        for (int R : rs)
            for (uint64_t k = 0; k < 1000; ++k) {
                int dy, dx;
                jitter_shift(seed, k, R, &dy, &dx);
                printf("shift %llu %d %llu -> %d %d\n", (unsigned long long)seed, R, (unsigned long long)k, dy, dx);
            }
    {   // a step counter far along: the multiplication wraps, nothing else does
        int dy, dx;
        jitter_shift(0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFEull, 4096, &dy, &dx);
        printf("shift %llu %d %llu -> %d %d\n", 0xFFFFFFFFFFFFFFFFull, 4096, 0xFFFFFFFFFFFFFFFEull, dy, dx);
    }

    const int ds[] = {0, 1, -1, 5, -5, 7, -7, 8, 300, -40, INT_MAX, INT_MIN, INT_MIN + 1};
    const int ns[] = {1, 7, 8, 4096, INT_MAX};
    for (int d : ds)
        for (int n : ns) printf("reduce %d %d -> %d\n", d, n, jitter_reduce(d, n));

    for (int H = 1; H <= 40; ++H)
        for (int W = 1; W <= 40; ++W) {
            const int shifts[6][2] = {{0, 0}, {1, 0}, {0, -1}, {-3, 2}, {H, W}, {-40, 300}};
            for (const auto& s : shifts) if (roll_case(H, W, s[0], s[1])) return 1;
        }
    // more rows than one trip of the planned grid covers are out of a host test's reach: a smaller grid makes the row loop take further trips
    if (roll_case(1000, 4, 999, 3) || roll_case(333, 5, -1, -1) || roll_case(1000, 4, 999, 3, 7) || roll_case(333, 5, -1, -1, 1)) return 1;
    {
        JitterPlan p;
        if (jitter_plan(0, 5, 0, 0, &p) != JITTER_SIZE || jitter_plan(5, 0, 0, 0, &p) != JITTER_SIZE || jitter_plan(-1, 5, 0, 0, &p) != JITTER_SIZE ||
            jitter_plan(INT_MAX, 5, 0, 0, &p) != JITTER_SIZE) return 1;
        printf("plan_refused\n");
        // large images: the grids stay inside their caps and the sizes do not wrap (the second one needs the kernel's row loop)
        if (jitter_plan(8192, 8192, -5, 8191, &p) != JITTER_OK) return 1;
        printf("big %d %u %u %u %u %zu\n", p.rows, p.gx, p.gy, p.gx_vec, p.gy_vec, p.pixels);
        if (jitter_plan(400000, 40000, 1, 1, &p) != JITTER_OK) return 1;
        printf("big %d %u %u %u %u %zu\n", p.rows, p.gx, p.gy, p.gx_vec, p.gy_vec, p.pixels);
    }
    return 0;
}
