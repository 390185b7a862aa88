// metrics_env.h — per-episode trajectory metrics for envs that restart on their own
// (pmenv_metrics_episodes; the contract is in include/pmenv.h).
//
// The lockstep kernel's geometry (replay.h, metrics_fused_kernel) with segment state per
// lane: blocks [0, nseg) walk returns / values / dones with lane = env and the horizon
// split over the four waves of a workgroup, blocks [nseg, nseg + nturn) stream the
// weights element-parallel, both in one launch. Step t (1 .. T) reads returns row t - 1,
// dones row t - 1 and values / weights row t.
//
// Segment walk. Wave w owns steps (c0, c1] = (T w / 4, T (w + 1) / 4].
//   A  each wave counts its chunk's dones and notes the first and the last one; through
//      LDS every wave then knows the dones of the earlier chunks (its first output slot
//      k0), the step e the episode in flight at c0 began after, and the column's count.
//   B  the wave walks its chunk once. The episode in flight at c0 (the head) is summed
//      with the shift K = its first excess return, returns[e] - rfp, which the wave reads
//      itself: every chunk of one episode uses the same K, so their shifted sums add
//      without a correction. An episode that begins in the chunk takes K from its first
//      step, starts its peak at init_value and is emitted where it ends; the episode
//      still open at c1 (the tail) leaves its sums, peak and drawdown in LDS.
//   C  the drawdown of the head needs the peak of what came before: the wave re-walks its
//      head (an L2 re-read, as metrics_seg_body re-walks its segment) with the peak
//      seeded from the tail that began the episode and the whole chunks between.
//   D  the wave in whose chunk the head ends (or wave 3, for the open episode that ends
//      at T) adds the parts in chronological order: the tail of the chunk with the
//      latest earlier done, the whole chunks after it, its own head.
// With dones = 0 this is metrics_seg_body's walk and its order of additions.
//
// Turnover. A workgroup owns eb whole envs, one thread per (env, asset), the previous
// weight in a register; at an episode end the env's threads add their partials in asset
// order: by shuffles where an env fits a wave (N <= 64: no barrier, no LDS), through an
// LDS slab and two barriers per kMeKC rows above (see the two bodies).
// No atomics anywhere: the same bits on every call and for every max_episodes.
#pragma once
#include "common.h"

namespace pmenv_dev {

constexpr int kMeKC = 8;                          // rows per turnover block
constexpr int kMeShDoubles = 12 * 256;            // the walk's 10 f64 + 4 int32 per (wave, lane); the slab is 8 x 256

__device__ __forceinline__ void metrics_env_emit(double* __restrict__ out, int32_t* __restrict__ span, size_t slot,
                                                 double K, int n, double s1, double s2, double dn, double mdd,
                                                 double vlast, int first, int last, double sqp) {
    const double mean = K + s1 / n;
    const double sd = n > 1 ? sqrt(fmax(s2 - s1 * s1 / n, 0.0) / (n - 1)) : NAN;
    double* o = out + slot * 5;
    o[0] = mean / sd * sqp;
    o[1] = mean / sqrt(dn / n) * sqp;
    o[2] = mdd;
    o[4] = vlast;
    span[slot * 2] = first;
    span[slot * 2 + 1] = last;
}

__device__ __forceinline__ void metrics_env_seg_body(const double* __restrict__ returns,
                                                     const double* __restrict__ values,
                                                     const uint8_t* __restrict__ dones, int T, int B, double init_value,
                                                     double rf, double periods, int KE, double* __restrict__ out,
                                                     int32_t* __restrict__ span, int32_t* __restrict__ count, int bid,
                                                     double* shd) {
    // [4][64] each: head S1, S2, down, max; tail S1, S2, down, peak, mdd; head mdd; then ints
    double(*sh)[4][64] = reinterpret_cast<double(*)[4][64]>(shd);
    int(*shi)[4][64] = reinterpret_cast<int(*)[4][64]>(shd + 10 * 256);   // dones, last done, head n, tail n
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = bid * 64 + lane;
    const bool ok = b < B;
    const int bb = ok ? b : B - 1;
    const double rfp = rf != 0.0 ? pow(1.0 + rf, 1.0 / periods) - 1.0 : 0.0;
    const double sqp = sqrt(periods);
    const int c0 = (int)((int64_t)T * w / 4), c1 = (int)((int64_t)T * (w + 1) / 4);
    const uint8_t* dcol = dones + bb;
    const double* rcol = returns + bb;
    const double* vcol = values + bb;

    // A: this chunk's dones
    int cn = 0, fd = 0, ld = 0;
    for (int t = c0 + 1; t <= c1; ++t) {
        if (dcol[(size_t)(t - 1) * B] != 0) {
            if (cn == 0) fd = t;
            ld = t;
            ++cn;
        }
    }
    shi[0][w][lane] = cn;
    shi[1][w][lane] = ld;
    __syncthreads();
    int k0 = 0, eprev = 0, total = 0, lastall = 0, j0 = -1;
    for (int j = 0; j < 4; ++j) {
        const int c = shi[0][j][lane], l = shi[1][j][lane];
        if (c != 0) {
            if (j < w) {
                eprev = l;
                j0 = j;
            }
            lastall = l;
        }
        if (j < w) k0 += c;
        total += c;
    }
    const int nep = total + (lastall != T ? 1 : 0);
    if (ok) {
        if (w == 3) count[b] = nep;
        for (int k = nep + w; k < KE; k += 4) {                  // the slots no episode takes
            const size_t slot = (size_t)b * KE + k;
#pragma unroll
            for (int f = 0; f < 5; ++f) out[slot * 5 + f] = NAN;
            span[slot * 2] = 0;
            span[slot * 2 + 1] = 0;
        }
    }

    // B: one walk of the chunk
    double K = rcol[(size_t)eprev * B] - rfp;
    double s1 = 0.0, s2 = 0.0, dn = 0.0, peak = -INFINITY, mdd = 0.0, vlast = 0.0;
    int n = 0, first = eprev + 1, li = 0;
    bool inhead = true;
    double hs1 = 0.0, hs2 = 0.0, hdn = 0.0, hmax = -INFINITY;
    int hn = 0;
    auto step = [&](int t, double x, double v, uint8_t d) {
        if (!inhead && n == 0) K = x;
        const double dd = x - K;
        s1 += dd;
        s2 += dd * dd;
        dn += x < 0.0 ? x * x : 0.0;
        ++n;
        peak = fmax(peak, v);
        if (!inhead) mdd = fmin(mdd, v / peak - 1.0);
        vlast = v;
        if (d != 0) {
            if (inhead) {
                hs1 = s1, hs2 = s2, hdn = dn, hmax = peak, hn = n;
                inhead = false;
            } else if (ok && k0 + li < KE) {
                metrics_env_emit(out, span, (size_t)b * KE + k0 + li, K, n, s1, s2, dn, mdd, v, first, t, sqp);
            }
            ++li;
            s1 = s2 = dn = mdd = 0.0;
            n = 0;
            peak = init_value;
            first = t + 1;
        }
    };
    int t = c0 + 1;
    for (; t + 3 <= c1; t += 4) {
        double x[4], v[4];
        uint8_t d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            x[u] = rcol[(size_t)(t + u - 1) * B] - rfp;
            v[u] = vcol[(size_t)(t + u) * B];
            d[u] = dcol[(size_t)(t + u - 1) * B];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) step(t + u, x[u], v[u], d[u]);
    }
    for (; t <= c1; ++t) step(t, rcol[(size_t)(t - 1) * B] - rfp, vcol[(size_t)t * B], dcol[(size_t)(t - 1) * B]);
    if (inhead) hs1 = s1, hs2 = s2, hdn = dn, hmax = peak, hn = n;      // no done: the chunk is all head
    else if (w == 3 && n > 0 && ok && k0 + li < KE)                       // the open episode began in this chunk
        metrics_env_emit(out, span, (size_t)b * KE + k0 + li, K, n, s1, s2, dn, mdd, vlast, first, T, sqp);
    sh[0][w][lane] = hs1;
    sh[1][w][lane] = hs2;
    sh[2][w][lane] = hdn;
    sh[3][w][lane] = hmax;
    sh[4][w][lane] = s1;
    sh[5][w][lane] = s2;
    sh[6][w][lane] = dn;
    sh[7][w][lane] = peak;
    sh[8][w][lane] = mdd;
    shi[2][w][lane] = hn;
    shi[3][w][lane] = n;
    __syncthreads();

    // C: the head's drawdown, the peak seeded by the episode's earlier chunks
    const int hend = cn != 0 ? fd : c1;
    double seed = j0 >= 0 ? sh[7][j0][lane] : vcol[0];
    for (int j = j0 + 1; j < w; ++j) seed = fmax(seed, sh[3][j][lane]);
    double hm = 0.0;
    for (t = c0 + 1; t <= hend; ++t) {
        const double v = vcol[(size_t)t * B];
        seed = fmax(seed, v);
        hm = fmin(hm, v / seed - 1.0);
    }
    sh[9][w][lane] = hm;
    __syncthreads();

    // D: the wave whose chunk ends the head folds the parts in chronological order
    if (!ok || !(cn != 0 || w == 3) || k0 >= KE) return;
    double S1 = 0.0, S2 = 0.0, DN = 0.0, MDD = 0.0;
    int Nn = 0;
    if (j0 >= 0) {
        S1 = sh[4][j0][lane], S2 = sh[5][j0][lane], DN = sh[6][j0][lane], MDD = sh[8][j0][lane];
        Nn = shi[3][j0][lane];
    }
    for (int j = j0 + 1; j <= w; ++j) {
        S1 += sh[0][j][lane];
        S2 += sh[1][j][lane];
        DN += sh[2][j][lane];
        MDD = fmin(MDD, sh[9][j][lane]);
        Nn += shi[2][j][lane];
    }
    metrics_env_emit(out, span, (size_t)b * KE + k0, rcol[(size_t)eprev * B] - rfp, Nn, S1, S2, DN, MDD,
                     vcol[(size_t)hend * B], eprev + 1, hend, sqp);
}

// N <= 64: an env's threads share a wave, so an episode's partials are added by shuffles in
// asset order and the stream runs without a barrier, as metrics_turnover_body's does
__device__ __forceinline__ void metrics_env_turnover_wave(const float* __restrict__ weights,
                                                          const uint8_t* __restrict__ dones, int T, int B, int N,
                                                          int epw, int KE, double* __restrict__ out, int bid) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int le = lane / N, el = lane - le * N;
    const int b = (bid * 4 + wv) * epw + le;
    if (le >= epw || b >= B) return;
    const int base = le * N;
    const size_t step = (size_t)B * N;
    const float* wc = weights + (size_t)b * N + el;
    const uint8_t* dcol = dones + b;
    float prev = wc[0];
    double acc = 0.0;
    int seg_first = 1, k = 0;
    auto row = [&](int t, float x, uint8_t d) {
        acc += fabs((double)x - (double)prev);
        prev = x;
        if (d != 0 || t == T) {                   // the env's threads take this branch together
            double tot = 0.0;
            for (int q = 0; q < N; ++q) tot += __shfl(acc, base + q);
            if (el == 0 && k < KE) out[((size_t)b * KE + k) * 5 + 3] = tot / (t - seg_first + 1);
            ++k;
            seg_first = t + 1;
            acc = 0.0;
            prev = el == 0 ? 1.0f : 0.0f;
        }
    };
    int t = 1;
    for (; t + 7 <= T; t += 8) {                  // eight rows in flight per thread
        float x[8];
        uint8_t d[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            x[u] = wc[(size_t)(t + u) * step];
            d[u] = dcol[(size_t)(t + u - 1) * B];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) row(t + u, x[u], d[u]);
    }
    for (; t <= T; ++t) row(t, wc[(size_t)t * step], dcol[(size_t)(t - 1) * B]);
}

// N > 64: an env's threads span waves (N > 256: one env per workgroup, threads stride over the
// assets and re-read the previous row). Time goes in blocks of kMeKC rows: at an episode end a
// thread puts its partial into the LDS slab [kMeKC][256] (at most kMeKC episodes end per env
// and block); after the block's barrier one thread per (env, ended episode) adds the env's
// partials in asset order, and a second barrier frees the slab.
__device__ __forceinline__ void metrics_env_turnover_slab(const float* __restrict__ weights,
                                                          const uint8_t* __restrict__ dones, int T, int B, int N,
                                                          int tpe, int eb, int KE, double* __restrict__ out, int bid,
                                                          double* slab) {
    const int tid = threadIdx.x;
    const int el = tid % tpe, le = tid / tpe;
    const int b = bid * eb + le;
    const bool active = le < eb && b < B;
    const bool multi = N > tpe;                   // N > 256: tpe = 256, eb = 1
    const size_t step = (size_t)B * N;
    const float* wc = weights + (size_t)(active ? b : 0) * N;
    const uint8_t* dcol = dones + (active ? b : 0);
    float prev = active && !multi ? wc[el] : 0.0f;
    bool fresh = false;                           // the previous row ended an episode
    double acc = 0.0;
    int seg_first = 1, kbase = 0;
    for (int t0 = 1; t0 <= T; t0 += kMeKC) {
        const int rows = min(kMeKC, T - t0 + 1);
        unsigned dm = 0;                          // bit i: row t0 + i ends an episode (T ends the open one)
        if (active) {
            uint8_t d[kMeKC];
            float x[kMeKC];
#pragma unroll
            for (int i = 0; i < kMeKC; ++i) {
                d[i] = i < rows ? dcol[(size_t)(t0 + i - 1) * B] : 0;
                x[i] = i < rows && !multi ? wc[(size_t)(t0 + i) * step + el] : 0.0f;
            }
            double* sl = slab + tid;
            int nd = 0;
#pragma unroll
            for (int i = 0; i < kMeKC; ++i) {
                if (i < rows) {
                    if (!multi) {
                        acc += fabs((double)x[i] - (double)prev);
                        prev = x[i];
                    } else {
                        const float* cur = wc + (size_t)(t0 + i) * step;
                        for (int a = el; a < N; a += tpe) {
                            const float p = fresh ? (a == 0 ? 1.0f : 0.0f) : (cur - step)[a];
                            acc += fabs((double)cur[a] - (double)p);
                        }
                    }
                    fresh = d[i] != 0;
                    if (fresh || t0 + i == T) {
                        sl[nd * 256] = acc;
                        ++nd;
                        dm |= 1u << i;
                        acc = 0.0;
                        prev = el == 0 ? 1.0f : 0.0f;
                    }
                }
            }
        }
        __syncthreads();
        if (active) {
            const double* sl = slab + le * tpe;
            int j = 0;
            for (int i = 0; i < kMeKC; ++i) {
                if ((dm >> i) & 1u) {
                    const int last = t0 + i, k = kbase + j;
                    if (j % tpe == el && k < KE) {
                        double tot = 0.0;
                        for (int q = 0; q < tpe; ++q) tot += sl[j * 256 + q];
                        out[((size_t)b * KE + k) * 5 + 3] = tot / (last - seg_first + 1);
                    }
                    seg_first = last + 1;
                    ++j;
                }
            }
            kbase += j;
        }
        __syncthreads();
    }
}

static __global__ __launch_bounds__(256) void metrics_env_fused_kernel(
    const double* __restrict__ returns, const double* __restrict__ values, const float* __restrict__ weights,
    const uint8_t* __restrict__ dones, int T, int B, int N, double init_value, double rf, double periods, int KE,
    int tpe, int eb, int nseg, double* __restrict__ out, int32_t* __restrict__ span, int32_t* __restrict__ count) {
    __shared__ double sh[kMeShDoubles];
    const int bid = (int)blockIdx.x;
    if (bid < nseg) metrics_env_seg_body(returns, values, dones, T, B, init_value, rf, periods, KE, out, span, count,
                                         bid, sh);
    else if (N <= 64) metrics_env_turnover_wave(weights, dones, T, B, N, eb / 4, KE, out, bid - nseg);
    else metrics_env_turnover_slab(weights, dones, T, B, N, tpe, eb, KE, out, bid - nseg, sh);
}

}  // namespace pmenv_dev
