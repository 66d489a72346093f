// csrc/color_match.h on the host, alone (no HIP, no engine), under the address and undefined-behaviour sanitizers
// (tests/test_color_match_cpu.py builds and runs it).  First the header's error returns; then every line of standard input -- 18 numbers
// (strtod: decimal or hex floats): mean_c[3] cov_c[6] mean_s[3] cov_s[6] -- is answered by one line "ok" + A[9] b[3] as hex floats, or
// "err <reason>".
#include "../style_transfer2_amd/csrc/color_match.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

static void error_returns()
{
    const double mean[3] = {120.0, 110.0, 100.0};
    const double cov[6] = {900.0, 100.0, 50.0, 800.0, 60.0, 700.0};
    float A[9], b[3];
    const char* why = nullptr;
    CHECK(st2c::color_transform(mean, cov, mean, cov, A, b, &why) == ST_OK);
    // the same moments on both sides: the identity map
    for (int i = 0; i < 9; ++i) CHECK(fabs((double)A[i] - (i % 4 == 0 ? 1.0 : 0.0)) <= 1e-6);
    for (int i = 0; i < 3; ++i) CHECK(fabs((double)b[i]) <= 1e-4);
    CHECK(st2c::color_transform(mean, cov, mean, cov, A, b, nullptr) == ST_OK);          // the reason is optional
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (int side = 0; side < 2; ++side)
        for (int i = 0; i < 9; ++i)
            for (double bad : {nan, inf, -inf}) {
                double m[3], c[6];
                memcpy(m, mean, sizeof m); memcpy(c, cov, sizeof c);
                if (i < 3) m[i] = bad; else c[i - 3] = bad;
                why = nullptr;
                const int rc = side ? st2c::color_transform(mean, cov, m, c, A, b, &why) : st2c::color_transform(m, c, mean, cov, A, b, &why);
                CHECK(rc == ST_ERR_ARG);
                CHECK(why && strstr(why, "not finite"));
            }
    for (int d : {0, 3, 5}) {
        double c[6];
        memcpy(c, cov, sizeof c);
        c[d] = -1.0;
        why = nullptr;
        CHECK(st2c::color_transform(mean, cov, mean, c, A, b, &why) == ST_ERR_ARG);
        CHECK(why && strstr(why, "negative diagonal"));
        CHECK(st2c::color_transform(mean, c, mean, cov, A, b, &why) == ST_ERR_ARG);
    }
    // a diagonal that is fine and off-diagonal entries no covariance has: no Cholesky factor, ridge or not
    const double broken[6] = {1.0, 500.0, 0.0, 1.0, 0.0, 1.0};
    why = nullptr;
    CHECK(st2c::color_transform(mean, cov, mean, broken, A, b, &why) == ST_ERR_ARG);
    CHECK(why && strstr(why, "Cholesky"));
    CHECK(st2c::color_transform(nullptr, cov, mean, cov, A, b, &why) == ST_ERR_ARG);
    // rank 1 (a grey image) and rank 0 (one flat colour): the ridge carries them
    const double grey[6] = {400.0, 400.0, 400.0, 400.0, 400.0, 400.0}, flat[6] = {0, 0, 0, 0, 0, 0};
    CHECK(st2c::color_transform(mean, cov, mean, grey, A, b, &why) == ST_OK);
    for (int i = 0; i < 9; ++i) CHECK(isfinite(A[i]));
    CHECK(st2c::color_transform(mean, flat, mean, grey, A, b, &why) == ST_OK);
    // moments_finish: two pixels (1, 2, 3) and (3, 2, 1) in preprocessed coordinates
    const double sums[9] = {4, 4, 4, 10, 8, 6, 8, 8, 10};
    double m[3], c[6];
    st2c::moments_finish(sums, 2.0, m, c);
    const double want[6] = {1, 0, -1, 0, 0, 1};
    for (int i = 0; i < 3; ++i) CHECK(m[i] == 2.0 + st2c::kMeanD[i]);
    for (int i = 0; i < 6; ++i) CHECK(c[i] == want[i]);
}

int main()
{
    error_returns();
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("all checks passed\n");
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        double v[18];
        char* p = line;
        int n = 0;
        for (; n < 18; ++n) {
            char* end = nullptr;
            v[n] = strtod(p, &end);
            if (end == p) break;
            p = end;
        }
        if (n != 18) { printf("err expected 18 numbers, got %d\n", n); continue; }
        float A[9], b[3];
        const char* why = "";
        if (st2c::color_transform(v, v + 3, v + 9, v + 12, A, b, &why) != ST_OK) { printf("err %s\n", why); continue; }
        printf("ok");
        for (int i = 0; i < 9; ++i) printf(" %a", (double)A[i]);
        for (int i = 0; i < 3; ++i) printf(" %a", (double)b[i]);
        printf("\n");
    }
    return 0;
}
