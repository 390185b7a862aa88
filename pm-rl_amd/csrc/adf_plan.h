// adf_plan.h — the search for the orders of differencing (data/ffd.py:59-78) on the host: the
// lag bound of the augmented Dickey-Fuller regression as an integer rule, MacKinnon's p-value,
// the bisection constants, and the geometry, the workspace and the names of the kernels of
// adf.h. pmenv_adf, pmenv_adf_workspace, pmenv_adf_path, pmenv_adf_maxlag and pmenv_adf_pvalue
// go through here, and the kernels call the same functions, so host and device cannot
// disagree on a column's lag bound. Host only and pure when a plain host compiler reads it:
// no HIP header, no HIP call (PMENV_HD is empty there), all products in int64.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/pmenv.h"

#if defined(__HIPCC__)
#define PMENV_HD __host__ __device__
#else
#define PMENV_HD
#endif

namespace pmenv_host {

constexpr int kAdfMaxLag = 64;     // the regressor cap: lags of one model (level and response come on top)
constexpr int kAdfMinRows = 16;    // fewer rows: PMENV_ADF_TOO_SHORT
constexpr int kAdfTile = 8;        // columns one workgroup of adf_sums_kernel stages (one wave each)
constexpr int kAdfChunk = 256;     // rows per staging step; the ring keeps two of them
constexpr int kAdfTableBlock = 64; // ffd_table_kernel: one lane per column

// adfuller's default maxlag (statsmodels' ceil(12 * (n / 100)^(1/4))) without a float: the
// smallest m with 100 m^4 >= 20736 n (12^4 = 20736), so n = 100, 1,600, 8,100 ... land on
// m = 12, 24, 36 exactly. Then min(n / 2 - 2, m). n < 4 gives 0.
PMENV_HD inline int64_t adf_rule(int64_t n) {
    if (n < 4) return 0;
    int64_t m = 0;
    while (100 * m * m * m * m < 20736 * n) ++m;       // n < 2^31: m < 820, the product < 2^46
    const int64_t half = n / 2 - 2;
    return m < half ? m : half;
}

// the lag bound of a column of n rows: the caller's maxlag >= 0 replaces the rule; either is
// clamped to n / 2 - 2 (and to 0 from below)
PMENV_HD inline int64_t adf_maxlag(int64_t n, int32_t maxlag) {
    if (maxlag < 0) return adf_rule(n);
    const int64_t half = n / 2 - 2;
    const int64_t k = maxlag < half ? maxlag : half;
    return k < 0 ? 0 : k;
}

// MacKinnon (1994), constant only, one series: the small-p polynomial up to -1.61, the
// large-p one above, Phi(z) = erfc(-z / sqrt 2) / 2
PMENV_HD inline double adf_pvalue(double s) {
    if (s != s) return s;
    if (s > 2.74) return 1.0;
    if (s < -18.83) return 0.0;
    const double z = s <= -1.61 ? 2.1659 + s * (1.4412 + s * 0.038269)
                                : 1.7339 + s * (0.93202 + s * (-0.12745 + s * -0.010368));
    return 0.5 * erfc(-z * 0.70710678118654752440);
}

// ---------------------------------------------------------------- the search's bracket rules
constexpr double kAdfPHigh = 0.05;    // p above: not stationary yet, low = d_mid
constexpr double kAdfPLow = 0.049;    // p below: stationary with room, high = d_mid

// ---------------------------------------------------------------- geometry and workspace
struct AdfPlan {
    bool ok = false;
    int kcap = 0;                 // the largest lag bound any column of the call can have
    int rec = 0;                  // doubles per column record: 2 kcap + 7
    size_t work_bytes = 0;
    unsigned sums_grid = 0, sums_block = 64 * kAdfTile;
    unsigned solve_grid = 0, solve_block = 64;
    unsigned solve_lds = 0;       // dynamic LDS bytes of adf_solve_kernel
};

// doubles of adf_solve_kernel's LDS for a lag cap k: the packed products of the k + 1
// difference columns, the packed Gram matrix under factorisation (k + 2 columns), and seven
// vectors of k + 2
PMENV_HD inline int64_t adf_solve_doubles(int64_t k) {
    return (k + 1) * (k + 2) / 2 + (k + 2) * (k + 3) / 2 + 7 * (k + 2);
}

// y [R, C] with row stride ld. Refused: R < 1, C < 1, ld < C, a lag bound above kAdfMaxLag
// (the caller's, or the rule's at n = R: series beyond 80,908 rows), a grid beyond 2^31 - 1.
inline AdfPlan adf_plan(int32_t R, int32_t C, int32_t ld, int32_t maxlag) {
    AdfPlan p;
    if (R < 1 || C < 1 || ld < C) return p;
    const int64_t kcap = adf_maxlag(R, maxlag);
    if (kcap > kAdfMaxLag || (maxlag > kAdfMaxLag)) return p;
    p.kcap = (int)kcap;
    p.rec = 2 * p.kcap + 7;          // the 2 k + 5 sums, the not-finite flag, the level's shift
    p.work_bytes = (size_t)C * (size_t)p.rec * sizeof(double);
    p.sums_grid = (unsigned)(((int64_t)C + kAdfTile - 1) / kAdfTile);
    p.solve_grid = (unsigned)C;
    p.solve_lds = (unsigned)(adf_solve_doubles(kcap) * (int64_t)sizeof(double));
    p.ok = true;
    return p;
}

// pmenv_adf_path's string: the two kernels in launch order with their geometry
inline void adf_plan_describe(const AdfPlan& p, char* out, size_t size) {
    if (size) out[0] = 0;
    if (!p.ok) return;
    snprintf(out, size,
             "adf_sums_kernel tile=%d chunk=%d kcap=%d grid=%u block=%u | adf_solve_kernel kcap=%d lds=%u grid=%u block=%u",
             kAdfTile, kAdfChunk, p.kcap, p.sums_grid, p.sums_block, p.kcap, p.solve_lds, p.solve_grid, p.solve_block);
}

}  // namespace pmenv_host
