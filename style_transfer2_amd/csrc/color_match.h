// Linear colour transfer on the host (st_color_transform, st_image_moments' finish): 3 x 3 closed form in double.  No HIP header here:
// tests/color_match_host_main.cpp compiles this file alone, under the host sanitizers.
#pragma once
#include "../../include/st2.h"

#include <math.h>

#include <initializer_list>

namespace st2c {
constexpr double kRidge = ST_COLOR_RIDGE;
// the channel mean of worker.py:34 as the kernels hold it (fp32), widened
constexpr double kMeanD[3] = {(double)123.68f, (double)116.779f, (double)103.939f};

// sums: {p_R, p_G, p_B, p_R p_R, p_R p_G, p_R p_B, p_G p_G, p_G p_B, p_B p_B} over n preprocessed pixels -> mean (image scale) and the
// upper triangle of the population covariance
inline void moments_finish(const double sums[9], double n, double mean[3], double cov[6])
{
    double m[3];
    for (int c = 0; c < 3; ++c) { m[c] = sums[c] / n; mean[c] = m[c] + kMeanD[c]; }
    int k = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b, ++k) cov[k] = sums[3 + k] / n - m[a] * m[b];
}

// cov (upper triangle RR, RG, RB, GG, GB, BB) + ridge I = L L^T, L lower triangular row-major; false: no factor (a pivot <= 0 or not finite)
inline bool cholesky3(const double cov[6], double ridge, double L[9])
{
    const double s00 = cov[0] + ridge, s01 = cov[1], s02 = cov[2], s11 = cov[3] + ridge, s12 = cov[4], s22 = cov[5] + ridge;
    for (int i = 0; i < 9; ++i) L[i] = 0.0;
    if (!(s00 > 0.0)) return false;
    L[0] = sqrt(s00);
    L[3] = s01 / L[0];
    L[6] = s02 / L[0];
    const double d1 = s11 - L[3] * L[3];
    if (!(d1 > 0.0)) return false;
    L[4] = sqrt(d1);
    L[7] = (s12 - L[6] * L[3]) / L[4];
    const double d2 = s22 - L[6] * L[6] - L[7] * L[7];
    if (!(d2 > 0.0)) return false;
    L[8] = sqrt(d2);
    for (int i = 0; i < 9; ++i) if (!isfinite(L[i])) return false;
    return true;
}

// A = L_c L_s^-1 and b = (mean_c - kMean) - A (mean_s - kMean), rounded once to fp32.  ST_OK, or ST_ERR_ARG with *why (nullable) set
inline int color_transform(const double mean_c[3], const double cov_c[6], const double mean_s[3], const double cov_s[6], float A[9], float b[3],
                           const char** why)
{
    const char* dummy;
    if (!why) why = &dummy;
    if (!mean_c || !cov_c || !mean_s || !cov_s || !A || !b) { *why = "a NULL argument"; return ST_ERR_ARG; }
    for (int i = 0; i < 3; ++i) if (!isfinite(mean_c[i]) || !isfinite(mean_s[i])) { *why = "a colour mean is not finite"; return ST_ERR_ARG; }
    for (int i = 0; i < 6; ++i) if (!isfinite(cov_c[i]) || !isfinite(cov_s[i])) { *why = "a covariance is not finite"; return ST_ERR_ARG; }
    for (int i : {0, 3, 5}) if (cov_c[i] < 0.0 || cov_s[i] < 0.0) { *why = "a covariance has a negative diagonal entry"; return ST_ERR_ARG; }
    double Lc[9], Ls[9], X[9];
    if (!cholesky3(cov_c, kRidge, Lc) || !cholesky3(cov_s, kRidge, Ls)) { *why = "a covariance (ridge added) has no Cholesky factor"; return ST_ERR_ARG; }
    // X L_s = L_c, row by row, last column first (L_s is lower triangular: column j of the product reads rows j .. 2 of L_s)
    for (int i = 0; i < 3; ++i) {
        X[i * 3 + 2] = Lc[i * 3 + 2] / Ls[8];
        X[i * 3 + 1] = (Lc[i * 3 + 1] - X[i * 3 + 2] * Ls[7]) / Ls[4];
        X[i * 3 + 0] = (Lc[i * 3 + 0] - X[i * 3 + 1] * Ls[3] - X[i * 3 + 2] * Ls[6]) / Ls[0];
    }
    for (int i = 0; i < 3; ++i) {
        double acc = mean_c[i] - kMeanD[i];
        for (int j = 0; j < 3; ++j) acc -= X[i * 3 + j] * (mean_s[j] - kMeanD[j]);
        b[i] = (float)acc;
    }
    for (int i = 0; i < 9; ++i) A[i] = (float)X[i];
    for (int i = 0; i < 9; ++i) if (!isfinite(A[i])) { *why = "the transform is not finite"; return ST_ERR_ARG; }
    for (int i = 0; i < 3; ++i) if (!isfinite(b[i])) { *why = "the transform is not finite"; return ST_ERR_ARG; }
    return ST_OK;
}
}  // namespace st2c
