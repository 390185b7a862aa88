// ffd_plan.h — the fractional-differencing filter of the feature pipeline on the host: the
// tap weights and width of one order d (data/ffd.py:38-47 as the reference's CPU path
// computes them), and the geometry and the name of the kernel that applies a tap table
// (features.h's ffd_apply_kernel). pmenv_ffd_weights, pmenv_ffd_apply and pmenv_ffd_path
// go through here, and so does the column scalers' partial geometry. Host only and pure:
// this header includes no HIP header and makes no HIP call (it compiles with a plain host
// compiler), and all products are taken in int64.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/pmenv.h"

namespace pmenv_host {

// ---------------------------------------------------------------- weights
// ffd.py:38-40: factor = zeros(T-1) - (d+1); proto = cat([1], factor / k + 1); weights =
// cumprod(proto). The factors are f32 throughout: (d+1) is rounded to f32 when it meets the
// f32 tensor, the division by k = 1 .. T-1 and the + 1 are f32 operations.
inline float ffd_factor(double d, int k) {
    const float neg = 0.0f - (float)(d + 1.0);
    const float q = neg / (float)k;
    return q + 1.0f;
}

// The taps of order d over a series of T rows: w_0 = 1, w_k = f32(prod_{i<=k} p_i) with the
// running product kept in f64 (the reference's CPU cumprod accumulates f32 in f64 and rounds
// every element once; a pure f32 product differs in the last bits), and the width
// ffd.py:43: max{k < T : |w_k| > thres}, the threshold rounded to f32 as the comparison with
// an f32 tensor does. Taps 0 .. width-1 are the filter (ffd.py:47 `weights[:width]` drops tap
// `width` itself: d = 1 is the single tap [1]); d = 0 is "leave the column alone", width 0
// (ffd.py:84). Writes min(width, cap) taps (taps may be NULL with cap = 0: the width only).
// PMENV_ERR_ARG: T < 2, d or thres negative or not finite, NULL width.
inline int ffd_weights(double d, double thres, int32_t T, float* taps, int32_t cap, int32_t* width) {
    if (!width || T < 2 || !(d >= 0.0) || !(thres >= 0.0) || !isfinite(d) || !isfinite(thres) || cap < 0 ||
        (cap > 0 && !taps))
        return PMENV_ERR_ARG;
    *width = 0;
    if (d == 0.0) return PMENV_OK;
    const float th = (float)thres;
    double prod = 1.0;
    int32_t w = 0;
    for (int32_t k = 1; k < T; ++k) {
        prod *= (double)ffd_factor(d, k);
        if (fabsf((float)prod) > th) w = k;
        if (prod == 0.0) break;                     // every later tap is 0 (integer d)
    }
    *width = w;
    prod = 1.0;
    for (int32_t k = 0; k < w && k < cap; ++k) {
        if (k) prod *= (double)ffd_factor(d, k);
        taps[k] = (float)prod;
    }
    return PMENV_OK;
}

// ---------------------------------------------------------------- the apply kernel's geometry
constexpr int kFfdRB = 8;       // consecutive outputs per lane (register block)
constexpr int kFfdJB = 8;       // taps per block: one block loads JB taps and JB new x rows for RB*JB FMAs
constexpr int kFfdWaves = 4;    // waves per workgroup, stacked in time

struct FfdPlan {
    bool ok = false;
    int cw_log2 = 0;            // columns per wave = 1 << cw_log2 (64 from 33 columns up)
    int cw = 0, slots = 0;      // columns per wave, time slots per wave (64 / cw)
    int rows = 0;               // output rows per workgroup: kFfdWaves * slots * kFfdRB
    unsigned grid_x = 0, grid_y = 0, block = 64 * kFfdWaves;   // x: time chunks, y: column groups
};

// x [T, C], out [T - max_width, C]. Lanes are columns (coalesced rows) — below 33 columns a
// wave holds 32 or 16 of them and its other lanes take further time slots (a single column
// still fills 4 lanes of a wave's 64; 16 keeps a workgroup's time chunk at 128 rows) — and
// every lane owns kFfdRB consecutive outputs of its column; the workgroup's waves sit on
// consecutive time chunks of the same columns. Refused (ok = false): T < 1, C < 1,
// max_width < 0, max_width >= T, or a grid beyond 2^31 - 1 x 65,535 workgroups.
inline FfdPlan ffd_plan(int32_t T, int32_t C, int32_t max_width) {
    FfdPlan p;
    if (T < 1 || C < 1 || max_width < 0 || max_width >= T) return p;
    int l = 4;
    while (l < 6 && (1 << l) < C) ++l;
    p.cw_log2 = l;
    p.cw = 1 << l;
    p.slots = 64 >> l;
    p.rows = kFfdWaves * p.slots * kFfdRB;
    const int64_t R = (int64_t)T - max_width;
    const int64_t gx = (R + p.rows - 1) / p.rows, gy = ((int64_t)C + p.cw - 1) / p.cw;
    if (gx > 0x7FFFFFFF || gy > 65535) return p;
    p.grid_x = (unsigned)gx;
    p.grid_y = (unsigned)gy;
    p.ok = true;
    return p;
}

// pmenv_ffd_path's string: the kernel as the library instantiates it, then its geometry
inline void ffd_plan_describe(const FfdPlan& p, char* out, size_t size) {
    if (size) out[0] = 0;
    if (!p.ok) return;
    snprintf(out, size, "ffd_apply_kernel<%d,%d> cw=%d slots=%d rows=%d grid=%ux%u block=%u", kFfdRB, kFfdJB, p.cw,
             p.slots, p.rows, p.grid_x, p.grid_y, p.block);
}

// ---------------------------------------------------------------- the scalers' geometry
constexpr int kScaleChunk = 256;   // rows per partial record of scale_fit (64 per wave of 4)

// partial records of a [T, C] fit: ceil(T / kScaleChunk) chunks (0: a refused shape)
inline int64_t scale_chunks(int32_t T, int32_t C) {
    if (T < 1 || C < 1) return 0;
    const int64_t n = ((int64_t)T + kScaleChunk - 1) / kScaleChunk;
    return n > 65535 || ((int64_t)C + 63) / 64 > 0x7FFFFFFF ? 0 : n;
}

// pmenv_scale_workspace: two doubles per (chunk, column)
inline size_t scale_workspace(int32_t T, int32_t C) {
    return (size_t)scale_chunks(T, C) * (size_t)(C > 0 ? C : 0) * 2 * sizeof(double);
}

}  // namespace pmenv_host
