// features.h — the feature pipeline's kernels: fixed-width-window fractional differencing
// over a tap table (data/ffd.py:80-89, the reference's per-column conv1d) and the per-column
// scalers (data/instrument.py:318-336: sklearn's MinMaxScaler / StandardScaler, one per
// (ticker, feature) column). x is [T, C] f32 with the C = N * (F-1) columns contiguous: the
// [T, N, F-1] bar layout. ffd_plan.h holds the weights and every geometry decision.
#pragma once

#include "common.h"
#include "ffd_plan.h"

namespace pmenv_dev {

using pmenv_host::kFfdWaves;
using pmenv_host::kScaleChunk;

// out[r, c] = sum_{j < width[c]} taps[j, c] * x[max_width + r - j, c], r < R = T - max_width.
// Each output is one f64 chain over its column's taps in ascending j, acc = fma((double)w_j,
// (double)x[t-j], acc) from acc = 0, rounded once to f32: the product of two f32 values is
// exact in f64, so the bits depend on no tiling. width 0 copies x[t]. A lane owns RB
// consecutive outputs of one column and walks the taps JB at a time: JB tap loads and JB new x
// rows feed RB * JB FMAs, the RB - 1 rows two tap blocks share stay in registers. Lanes of a
// wave may hold different widths: a tap block that lies inside every lane's width runs
// unpredicated, the others per lane. Rows and taps outside the tables are never read (the
// indices are clamped; what a clamped load returns is never used).
template <int RB, int JB>
static __global__ __launch_bounds__(64 * kFfdWaves) void ffd_apply_kernel(const float* __restrict__ x,
                                                                         const float* __restrict__ taps,
                                                                         const int32_t* __restrict__ width,
                                                                         float* __restrict__ out, int T, int C,
                                                                         int max_width, int cw_log2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cw = 1 << cw_log2, slots = 64 >> cw_log2;
    const int64_t R = (int64_t)T - max_width;
    const int64_t c_raw = (int64_t)blockIdx.y * cw + (lane & (cw - 1));
    const int64_t slot = ((int64_t)blockIdx.x * kFfdWaves + wave) * slots + (lane >> cw_log2);
    const int64_t r0 = slot * RB;
    const bool active = c_raw < C && r0 < R;
    const size_t c = (size_t)(c_raw < C ? c_raw : C - 1);
    int wc = 0;
    if (active) {
        wc = width[c];
        wc = wc < 0 ? 0 : (wc > max_width ? max_width : wc);
    }
    // the wave's largest width bounds the loop, the smallest positive one the unpredicated part
    int wmax = wc, wmin = wc > 0 ? wc : 0x7FFFFFFF;
    for (int o = 32; o > 0; o >>= 1) {
        wmax = max(wmax, __shfl_xor(wmax, o, 64));
        wmin = min(wmin, __shfl_xor(wmin, o, 64));
    }
    const int64_t t0 = max_width + r0;               // the series row of the lane's first output
    const int64_t last = (int64_t)T - 1;
    auto row = [&](int64_t t) { return (size_t)(t < 0 ? 0 : (t > last ? last : t)) * (size_t)C + c; };

    double acc[RB];
    double xs[RB + JB - 1];                          // xs[k] = x[t0 + RB-1 - j0 - k]: output i, tap j0+jj reads k = RB-1-i+jj
#pragma unroll
    for (int i = 0; i < RB; ++i) acc[i] = 0.0;
    if (wmax > 0) {
#pragma unroll
        for (int k = 0; k < RB - 1; ++k) xs[k] = (double)x[row(t0 + RB - 1 - k)];
    }
    for (int j0 = 0; j0 < wmax; j0 += JB) {
        double w[JB];
#pragma unroll
        for (int jj = 0; jj < JB; ++jj) {
            const int j = j0 + jj < max_width ? j0 + jj : max_width - 1;
            w[jj] = (double)taps[(size_t)j * (size_t)C + c];
            xs[RB - 1 + jj] = (double)x[row(t0 - j0 - jj)];
        }
        if (j0 + JB <= wmin) {
#pragma unroll
            for (int jj = 0; jj < JB; ++jj)
#pragma unroll
                for (int i = 0; i < RB; ++i) acc[i] = fma(w[jj], xs[RB - 1 - i + jj], acc[i]);
        } else {
#pragma unroll
            for (int jj = 0; jj < JB; ++jj)
                if (j0 + jj < wc) {
#pragma unroll
                    for (int i = 0; i < RB; ++i) acc[i] = fma(w[jj], xs[RB - 1 - i + jj], acc[i]);
                }
        }
#pragma unroll
        for (int k = 0; k < RB - 1; ++k) xs[k] = xs[k + JB];
    }
    if (!active) return;
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        if (r0 + i < R) {
            const size_t o = (size_t)(r0 + i) * (size_t)C + c;
            out[o] = wc > 0 ? (float)acc[i] : x[(size_t)(t0 + i) * (size_t)C + c];
        }
    }
}

// ---------------------------------------------------------------- the scalers' fit
// One workgroup folds kScaleChunk rows of 64 columns into one record per column,
// work[(chunk * C + c) * 2 + {0, 1}]: lanes are columns, wave w takes rows w, w + 4, ... of
// the chunk, and the four waves' values are folded in wave order. NaNs are skipped (sklearn's
// nanmin / nanmax / nanmean). MODE 0: {min, max}; 1: {sum, count}; 2: {sum of (x - mean)^2,
// count} with the mean read from stats[c]. f64 throughout, fixed row -> lane assignment:
// deterministic.
template <int MODE>
static __global__ __launch_bounds__(256) void scale_partial_kernel(const float* __restrict__ x, int T, int C,
                                                                   const double* __restrict__ stats,
                                                                   double* __restrict__ work) {
    __shared__ double sh[2][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * 64 + lane;
    const int64_t lo = (int64_t)blockIdx.y * kScaleChunk;
    const int64_t hi = lo + kScaleChunk < T ? lo + kScaleChunk : T;
    double a = MODE == 0 ? INFINITY : 0.0, b = MODE == 0 ? -INFINITY : 0.0;
    if (c < C) {
        const double mean = MODE == 2 ? stats[c] : 0.0;
        for (int64_t t = lo + wave; t < hi; t += 4) {
            const double v = (double)x[(size_t)t * (size_t)C + (size_t)c];
            if (v != v) continue;
            if (MODE == 0) {
                a = fmin(a, v);
                b = fmax(b, v);
            } else if (MODE == 1) {
                a += v;
                b += 1.0;
            } else {
                const double e = v - mean;
                a = fma(e, e, a);
                b += 1.0;
            }
        }
    }
    sh[0][wave][lane] = a;
    sh[1][wave][lane] = b;
    __syncthreads();
    if (wave == 0 && c < C) {
        for (int w = 1; w < 4; ++w) {
            const double a2 = sh[0][w][lane], b2 = sh[1][w][lane];
            if (MODE == 0) {
                a = fmin(a, a2);
                b = fmax(b, b2);
            } else {
                a += a2;
                b += b2;
            }
        }
        const size_t o = ((size_t)blockIdx.y * (size_t)C + (size_t)c) * 2;
        work[o] = a;
        work[o + 1] = b;
    }
}

// One thread per column folds the chunk records in chunk order into stats [2, C]. MODE 0:
// stats = {min, max} (NaN for a column without a number); 1: stats[0] = mean = sum / count;
// 2: stats[1] = sqrt(sum of squares / count), ddof 0.
template <int MODE>
static __global__ __launch_bounds__(256) void scale_final_kernel(int chunks, int C, const double* __restrict__ work,
                                                                 double* __restrict__ stats) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double a = MODE == 0 ? INFINITY : 0.0, b = MODE == 0 ? -INFINITY : 0.0;
    for (int k = 0; k < chunks; ++k) {
        const size_t o = ((size_t)k * (size_t)C + (size_t)c) * 2;
        if (MODE == 0) {
            a = fmin(a, work[o]);
            b = fmax(b, work[o + 1]);
        } else {
            a += work[o];
            b += work[o + 1];
        }
    }
    if (MODE == 0) {
        const bool none = a > b;
        stats[c] = none ? (double)NAN : a;
        stats[(size_t)C + c] = none ? (double)NAN : b;
    } else if (MODE == 1) {
        stats[c] = a / b;
    } else {
        stats[(size_t)C + c] = sqrt(a / b);
    }
}

// y = f32(((double)x - s0) / den): min-max s0 = min, den = max - min; standard s0 = mean,
// den = std; den == 0 divides by 1 (sklearn's _handle_zeros_in_scale). A NaN passes through.
// y may be x: every element is read and written by the same thread.
static __global__ __launch_bounds__(256) void scale_apply_kernel(const float* x, int T, int C, int standard,
                                                                 const double* __restrict__ stats, float* y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.y * 64 + lane;
    if (c >= C) return;
    const double s0 = stats[c], s1 = stats[(size_t)C + c];
    double den = standard ? s1 : s1 - s0;
    if (den == 0.0) den = 1.0;
    const int64_t lo = ((int64_t)blockIdx.x * 4 + wave) * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t t = lo + i;
        if (t < T) {
            const size_t o = (size_t)t * (size_t)C + (size_t)c;
            y[o] = (float)(((double)x[o] - s0) / den);
        }
    }
}

}  // namespace pmenv_dev
