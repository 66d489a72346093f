// Jitter (include/st2.h: st_set_jitter): validation of the radius, the shift sequence, the reduction of a shift, the source index of a
// rolled pixel and the launch grids of roll_k.  The engine (engine_jitter.cpp) and the launcher (jitter.hip) both ask here.  No HIP
// header: tests/jitter_plan_host_main.cpp compiles this file alone, under the host sanitizers.
#pragma once
#include "../../include/st2.h"

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ST2_JIT_HD __host__ __device__
#else
#define ST2_JIT_HD
#endif

namespace st2 {
constexpr int kJitterMaxRadius = 4096;
// roll_k's workgroup: kJitBlockX lanes along a row (one wave), kJitBlockY rows; a thread takes kJitRows rows per trip, kJitBlockY apart
constexpr int kJitBlockX = 64, kJitBlockY = 4, kJitRows = 4;
constexpr int kJitTripRows = kJitBlockY * kJitRows;        // rows one workgroup covers per trip
constexpr int kJitMaxGridY = 65535;

enum JitterRefusal { JITTER_OK = 0, JITTER_RADIUS, JITTER_SIZE };

inline const char* jitter_refusal_text(int r)
{
    switch (r) {
    case JITTER_OK: return "ok";
    case JITTER_RADIUS: return "the radius must be 0 (off) or inside [1, 4096]";
    case JITTER_SIZE: return "the image must be at least 1 x 1";
    }
    return "?";
}

inline int jitter_validate_radius(int radius) { return (radius < 0 || radius > kJitterMaxRadius) ? JITTER_RADIUS : JITTER_OK; }

// splitmix64's output function; all arithmetic wraps mod 2^64
inline uint64_t jitter_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// output k + 1 of splitmix64 started at `seed`
inline uint64_t jitter_draw(uint64_t seed, uint64_t k) { return jitter_mix(seed + (k + 1) * 0x9E3779B97F4A7C15ull); }

// the shift of step k: both components uniform over [-R, R] (up to the bias of the modulus), dy from the high word, dx from the low one
inline void jitter_shift(uint64_t seed, uint64_t k, int radius, int* dy, int* dx)
{
    const uint64_t r = jitter_draw(seed, k), span = 2ull * (uint64_t)radius + 1;
    *dy = (int)((r >> 32) % span) - radius;
    *dx = (int)((r & 0xFFFFFFFFull) % span) - radius;
}

// any integer shift -> the equivalent one inside [0, n)
inline int jitter_reduce(int d, int n)
{
    const long long m = (long long)d % n;
    return (int)(m < 0 ? m + n : m);
}

// roll(P, d)[i] = P[jitter_src(i, d, n)] along an axis of n elements, for a REDUCED d (0 <= d < n) and 0 <= i < n.  The one place that
// says which way a roll moves: the kernel, the launcher's checks and the host test all go through it
ST2_JIT_HD inline int jitter_src(int i, int d, int n)
{
    const int s = i - d;
    return s < 0 ? s + n : s;
}

struct JitterPlan {
    int H, W;
    int dy, dx;             // the reduced shift
    size_t plane;           // H * W
    size_t pixels;          // 3 * H * W: floats of either side
    int rows;               // 3 * H: rows of the three planes, back to back
    bool row_vec;           // W % 4 == 0: four consecutive destination pixels stay inside a row (the launcher adds the pointer tests)
    unsigned gx, gy;        // scalar form: a lane takes one pixel of a row
    unsigned gx_vec, gy_vec;// 16-byte form: a lane takes four consecutive pixels of a row
};

inline unsigned jitter_grid_y(int rows)
{
    const long long g = ((long long)rows + kJitTripRows - 1) / kJitTripRows;
    return (unsigned)(g > kJitMaxGridY ? kJitMaxGridY : g);         // (more rows than the grid covers: the kernel's row loop takes further trips)
}

inline int jitter_plan(int H, int W, int dy, int dx, JitterPlan* out)
{
    if (H < 1 || W < 1 || (long long)H * 3 > 0x7FFFFFFFll) return JITTER_SIZE;
    JitterPlan p{};
    p.H = H; p.W = W;
    p.dy = jitter_reduce(dy, H); p.dx = jitter_reduce(dx, W);
    p.plane = (size_t)H * W;
    p.pixels = 3 * p.plane;
    p.rows = 3 * H;
    p.row_vec = W % 4 == 0;
    p.gx = (unsigned)((W + kJitBlockX - 1) / kJitBlockX);
    p.gx_vec = (unsigned)((W / 4 + kJitBlockX - 1) / kJitBlockX);
    if (p.gx_vec < 1) p.gx_vec = 1;
    p.gy = p.gy_vec = jitter_grid_y(p.rows);
    *out = p;
    return JITTER_OK;
}
}  // namespace st2
