// replay.h — device replay gather and trajectory metrics.
//
// replay_gather_kernel restates replay/buffer.py:39-79 (ReplayBuffer.sample) for
// vectorised envs: the buffer keeps, per recorded step h and env b, only the day
// index of the window the agent acted on, the action and the reward; a sample
// (h0, b) re-materialises
//   s  = window ending at day[h0+W-1, b]      with channel F-1 = actions[h0 .. h0+W-1, b]
//   s' = window ending at day[h0+W-1, b] + 1  with channel F-1 = actions[h0+1 .. h0+W, b]
//   a  = actions[h0+W, b],  r = rewards[h0+W-1, b]                (buffer.py:59-72)
// from the resident market series [T, N, F-1]. Recorded steps are a ring of H rows.
// The replay_nstep_* kernels fold up to n such transitions into one at sample time
// (agent/td3/td3.py:85-106): see "n-step samples" below. The replay_seq_* kernels serve
// sequences of consecutive samples (agent/dreamer/dreamer.py:77-80): "sequence samples".
//
// metrics_kernel restates util/eval.py:14-37 per env over a [T, B] trajectory with
// quantstats' published definitions (quantstats is not installed here: parity unpinned).
#pragma once
#include "common.h"

namespace pmenv_dev {

// one thread per output float of s and s' (both [S, N, W, F]); a/r by the first threads
static __global__ void replay_gather_kernel(const float* series, int T, int N, int F, int W, const int32_t* days,
                                     const float* actions, const float* rewards, int H, int B, const int32_t* h0,
                                     const int32_t* env, int S, float* s, float* s_next, float* a_out,
                                     float* r_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per = (int64_t)N * W * F;
    const int Fm = F - 1;
    if (i < (int64_t)S * N) {                     // a = actions[h0+W], r = rewards[h0+W-1]
        const int j = (int)(i / N), n = (int)(i % N);
        const int b = env[j];
        const int ha = (h0[j] + W) % H;
        a_out[i] = actions[((size_t)ha * B + b) * N + n];
        if (n == 0) r_out[j] = rewards[(size_t)((h0[j] + W - 1) % H) * B + b];
    }
    if (i >= (int64_t)S * per) return;
    const int j = (int)(i / per);
    int rem = (int)(i - (int64_t)j * per);
    const int n = rem / (W * F);
    rem -= n * W * F;
    const int t = rem / F, f = rem - t * F;
    const int b = env[j];
    const int hl = (h0[j] + W - 1) % H;           // the step whose window is s
    const int dlast = days[(size_t)hl * B + b];
    float v, vn;
    if (f < Fm) {
        const int d = dlast - (W - 1) + t;        // window of day dlast, and of dlast + 1 for s'
        v = (d >= 0 && d < T) ? series[((size_t)d * N + n) * Fm + f] : NAN;
        vn = (d + 1 >= 0 && d + 1 < T) ? series[((size_t)(d + 1) * N + n) * Fm + f] : NAN;
    } else {
        v = actions[((size_t)((h0[j] + t) % H) * B + b) * N + n];
        vn = actions[((size_t)((h0[j] + t + 1) % H) * B + b) * N + n];
    }
    s[i] = v;
    s_next[i] = vn;
}

// The compact on-policy rollout (the device rollout keeps actions,
// rewards and values, not windows): env b's window after t steps is re-materialised
// from the resident market series and the env's post-drift weight history —
//   market f < F-1:  series[start[b] + t + p, n, f]          (p = day in the window)
//   weight f = F-1:  ActionBuffer.get_all() after t updates (weight_buffer.py:32-44)
// with the history rows r = 0 .. T_rec+W-1 of env b: rows < W-1 zero, row W-1 = e0 (the
// reset ring, weight_buffer.py:46-51), row W-1+j = w' of update j (weights [T_rec, B, N]).
// Chronological position c of the window after u = t updates reads row t + c; once the
// ring is full (u >= W-1) the reference returns it in storage order (:38-39): position
// p holds update j with j % W == p, i.e. chronological c = (p - u - 1) mod W.
// Days outside the series read NaN.

constexpr int kRowGatherUnroll = 8;   // rows of W*F <= 512 floats: all loads first

// The per-env form of the map (pmenv_rollout_gather_env: envs that restart on their own, and
// rollouts that resume): the window (t, b) starts at day first[t, b] and has seen
// u = updates[t, b] ring updates since its env's last reset, so its history row is
// r = u + c, rows < W-1 zero and row W-1 = e0 as above, and a row r > W-1 is the w' of step
// t + c - W + 1 of this rollout: weights row carry + t + c - W ([carry + T_rec, B, N], the
// first `carry` rows the steps before the rollout began). Lockstep is first = start + t,
// u = t, carry = 0. What one sample's window depends on:
struct RolloutWin {
    int d0;         // series day of the window's first day
    int u;          // ring updates since the env's last reset
    int shift;      // weights row of history row r: r - W + shift (carry + t - u; lockstep 0)
    int rows;       // weights rows there are (the per-env form's upper guard)
    bool storage;   // the ring is full and read in storage order
};
__device__ __forceinline__ RolloutWin rollout_win_lockstep(const int32_t* start, int W, int ring_mode, int b, int t) {
    return RolloutWin{start[b] + t, t, 0, 0, ring_mode == PMENV_RING_STORAGE && t >= W - 1};
}
__device__ __forceinline__ RolloutWin rollout_win_env(const int32_t* first, const int32_t* updates, int carry,
                                                      int T_rec, int W, int B, int ring_mode, int b, int t) {
    const size_t at = (size_t)t * B + b;
    const int u = updates[at];
    return RolloutWin{first[at], u, carry + t - u, carry + T_rec, ring_mode == PMENV_RING_STORAGE && u >= W - 1};
}
// the weight channel at window position p. ENV: a row outside the recorded history reads 0
// (the lockstep rows are in range by r > W-1)
template <bool ENV>
__device__ __forceinline__ float rollout_weight(const RolloutWin& w, const float* weights, int W, int B, int N,
                                                int b, int n, int p) {
    const int c = w.storage ? (((p - w.u - 1) % W) + W) % W : p;
    const int r = w.u + c;                         // history row
    if (r < W - 1) return 0.0f;
    if (r == W - 1) return n == 0 ? 1.0f : 0.0f;
    if (!ENV) return weights[((size_t)(r - W) * B + b) * N + n];
    const int row = r - W + w.shift;
    if (row < 0 || row >= w.rows) return 0.0f;
    return weights[((size_t)row * B + b) * N + n];
}

// The map above, one wave per (sample, asset) row of W*F floats: a lane writes floats
// lane, lane + 64, ... of the row (each store one contiguous 256-B run), the day and
// channel from the row offset by one multiply-shift, the sample's env / step / start
// wave-uniform. The float-per-thread form (tools build) spends its time in 64-bit divisions.
template <bool ENV>
__device__ __forceinline__ void rollout_gather_rows_body(const float* series, int T, int N, int F, int W,
                                                         const RolloutWin& win, const float* weights, int B, int b,
                                                         int n, int lane, float* out, FastDiv div_f) {
    const int d0 = win.d0;
    const int Fm = F - 1, WF = W * F;
    // the value of row float i: a series or a weight-history float, or a constant
    auto fetch = [&](int i) -> float {
        const int p = (int)fdiv((uint32_t)i, div_f), f = i - p * F;
        if (f < Fm) {
            const int d = d0 + p;
            return (d >= 0 && d < T) ? series[((size_t)d * N + n) * Fm + f] : NAN;
        }
        return rollout_weight<ENV>(win, weights, W, B, N, b, n, p);
    };
    if (WF <= 64 * kRowGatherUnroll) {             // every load of the row in flight before the stores
        float v[kRowGatherUnroll];
#pragma unroll
        for (int k = 0; k < kRowGatherUnroll; ++k) v[k] = lane + 64 * k < WF ? fetch(lane + 64 * k) : 0.0f;
#pragma unroll
        for (int k = 0; k < kRowGatherUnroll; ++k)
            if (lane + 64 * k < WF) out[lane + 64 * k] = v[k];
        return;
    }
    for (int i = lane; i < WF; i += 64) out[i] = fetch(i);
}

static __global__ __launch_bounds__(256) void rollout_gather_rows_kernel(const float* series, int T, int N, int F, int W,
                                                                  const int32_t* start, const float* weights,
                                                                  int B, int ring_mode, const int32_t* t_idx,
                                                                  const int32_t* env, int S, float* s, FastDiv div_f) {
    const int64_t rowi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (rowi >= (int64_t)S * N) return;
    const int lane = threadIdx.x & 63;
    const int j = __builtin_amdgcn_readfirstlane((int)(rowi / N));
    const int n = __builtin_amdgcn_readfirstlane((int)(rowi - (int64_t)j * N));
    const int b = env[j], t = t_idx[j];
    rollout_gather_rows_body<false>(series, T, N, F, W, rollout_win_lockstep(start, W, ring_mode, b, t), weights, B,
                                    b, n, lane, s + rowi * (W * F), div_f);
}
// the per-env form: first / updates [T_rec + 1, B] in place of start, weights [carry + T_rec, B, N]
static __global__ __launch_bounds__(256) void rollout_gather_env_rows_kernel(
    const float* series, int T, int N, int F, int W, const int32_t* first, const int32_t* updates,
    const float* weights, int carry, int T_rec, int B, int ring_mode, const int32_t* t_idx, const int32_t* env, int S,
    float* s, FastDiv div_f) {
    const int64_t rowi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (rowi >= (int64_t)S * N) return;
    const int lane = threadIdx.x & 63;
    const int j = __builtin_amdgcn_readfirstlane((int)(rowi / N));
    const int n = __builtin_amdgcn_readfirstlane((int)(rowi - (int64_t)j * N));
    const int b = env[j], t = t_idx[j];
    rollout_gather_rows_body<true>(series, T, N, F, W,
                                   rollout_win_env(first, updates, carry, T_rec, W, B, ring_mode, b, t), weights, B, b,
                                   n, lane, s + rowi * (W * F), div_f);
}

// One workgroup per sample (F = 5, the sample's [W, N] weight block and [W, N, 4] market
// block fit LDS): both blocks are staged with coalesced reads — the market block is W
// consecutive series days, contiguous in [T, N, 4]; each history row's N weights are one
// contiguous run of [T_rec, B, N] — and the [N, W, 5] window is written as 16-B chunks
// from LDS (a lane's four floats walk (asset, day, channel) incrementally). Every weight
// line is fetched once per sample, where the per-row form fetches it per asset row.
// NT: cache-policy bits of the window stores (0: plain stores; the product: 16, sc1, for
// windows <= 128 MiB, else 2, nt; the tools build A/Bs the others)
template <int NT, bool ENV>
__device__ __forceinline__ void rollout_gather_tile_body(const float* series, int T, int N, int W,
                                                         const RolloutWin& win, const float* weights, int B, int b,
                                                         int j, float* s, FastDiv div_n, FastDiv div_wf,
                                                         FastDiv div_f) {
    constexpr int F = 5;
    extern __shared__ __attribute__((aligned(16))) float sh[];   // market [W][N][4], then weights [W][N]
    float* sh_m = sh;
    float* sh_w = sh + (size_t)W * N * 4;
    const int tid = threadIdx.x;
    const int d0 = win.d0;
    const int nd = W * N;                          // market: one f4 per (day, asset); weights: one float
    const f4* src = reinterpret_cast<const f4*>(series) + (size_t)d0 * N;
    f4* sh_m4 = reinterpret_cast<f4*>(sh_m);
    // every load of a round in flight before its LDS writes (4 per thread and array)
    for (int i0 = 0; i0 < nd; i0 += 4 * 256) {
        f4 m[4];
        float w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k * 256 + tid;
            m[k] = f4{NAN, NAN, NAN, NAN};
            w[k] = 0.0f;
            if (i < nd) {
                const int p = (int)fdiv((uint32_t)i, div_n), n = i - p * N;
                const int d = d0 + p;
                if (d >= 0 && d < T) m[k] = src[i];        // days outside the series read NaN
                w[k] = rollout_weight<ENV>(win, weights, W, B, N, b, n, p);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k * 256 + tid;
            if (i < nd) {
                sh_m4[i] = m[k];
                sh_w[i] = w[k];
            }
        }
    }
    __syncthreads();
    const int WF = W * F;
    const int nq = N * WF / 4;
    f4* out = reinterpret_cast<f4*>(s + (size_t)j * N * WF);
    for (int q = tid; q < nq; q += 256) {
        const int e = 4 * q;
        int n = (int)fdiv((uint32_t)e, div_wf);
        int rem = e - n * WF;
        int p = (int)fdiv((uint32_t)rem, div_f);
        int f = rem - p * F;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = f < F - 1 ? sh_m[(p * N + n) * 4 + f] : sh_w[p * N + n];
            if (++f == F) {
                f = 0;
                if (++p == W) {
                    p = 0;
                    ++n;
                }
            }
        }
        if constexpr (NT == 0) out[q] = f4{v[0], v[1], v[2], v[3]};
        else buf_store4<NT>(make_rsrc(out, (uint32_t)nq * 16u), (uint32_t)q * 16u, f4{v[0], v[1], v[2], v[3]});
    }
}

template <int NT = 0>
__global__ __launch_bounds__(256) void rollout_gather_tile_kernel(const float* series, int T, int N, int W,
                                                                  const int32_t* start, const float* weights, int B,
                                                                  int ring_mode, const int32_t* t_idx,
                                                                  const int32_t* env, float* s, FastDiv div_n,
                                                                  FastDiv div_wf, FastDiv div_f) {
    const int j = blockIdx.x;
    const int b = env[j], t = t_idx[j];
    rollout_gather_tile_body<NT, false>(series, T, N, W, rollout_win_lockstep(start, W, ring_mode, b, t), weights, B,
                                        b, j, s, div_n, div_wf, div_f);
}
// the per-env form, as rollout_gather_env_rows_kernel
template <int NT = 0>
__global__ __launch_bounds__(256) void rollout_gather_env_tile_kernel(
    const float* series, int T, int N, int W, const int32_t* first, const int32_t* updates, const float* weights,
    int carry, int T_rec, int B, int ring_mode, const int32_t* t_idx, const int32_t* env, float* s, FastDiv div_n,
    FastDiv div_wf, FastDiv div_f) {
    const int j = blockIdx.x;
    const int b = env[j], t = t_idx[j];
    rollout_gather_tile_body<NT, true>(series, T, N, W,
                                       rollout_win_env(first, updates, carry, T_rec, W, B, ring_mode, b, t), weights,
                                       B, b, j, s, div_n, div_wf, div_f);
}



// The same per-env metrics with the horizon split over the four waves of a
// workgroup (lane = env: every load is a coalesced 512-B row; four times the waves
// in flight of the thread-per-env walk). Wave w walks days [w*T/4, (w+1)*T/4):
//   sharpe / sortino: shifted sums S1 = sum(x - K), S2 = sum((x - K)^2) with K the
//   env's first excess return (no division in the loop), and sum(min(x, 0)^2);
//   max drawdown: each wave's segment maximum goes through LDS, then the wave
//   re-walks its segment (an L2 re-read) with the running peak seeded by the
//   maximum of every earlier segment.
// Wave 0 adds the four segments' sums in wave order: deterministic.
__device__ __forceinline__ void metrics_seg_body(const double* returns, const double* values, int T, int B, double rf,
                                                 double periods, double* out, int bid) {
    __shared__ double sh[5][4][64];              // S1, S2, down, segment max (of values), mdd
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = bid * 64 + lane;
    const bool ok = b < B;
    const int bb = ok ? b : B - 1;
    const double rfp = rf != 0.0 ? pow(1.0 + rf, 1.0 / periods) - 1.0 : 0.0;
    const double K = returns[bb] - rfp;
    // returns: T rows, values: T + 1 rows; split both the same way
    const int r0 = (int)((int64_t)T * w / 4), r1 = (int)((int64_t)T * (w + 1) / 4);
    double s1 = 0.0, s2 = 0.0, dn = 0.0;
    int t = r0;
    for (; t + 4 <= r1; t += 4) {
        double x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = returns[(size_t)(t + u) * B + bb] - rfp;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double d = x[u] - K;
            s1 += d;
            s2 += d * d;
            dn += x[u] < 0.0 ? x[u] * x[u] : 0.0;
        }
    }
    for (; t < r1; ++t) {
        const double x = returns[(size_t)t * B + bb] - rfp;
        const double d = x - K;
        s1 += d;
        s2 += d * d;
        dn += x < 0.0 ? x * x : 0.0;
    }
    const int v0 = (int)((int64_t)(T + 1) * w / 4), v1 = (int)((int64_t)(T + 1) * (w + 1) / 4);
    double vmax = -INFINITY;
    for (t = v0; t < v1; ++t) vmax = fmax(vmax, values[(size_t)t * B + bb]);
    sh[0][w][lane] = s1;
    sh[1][w][lane] = s2;
    sh[2][w][lane] = dn;
    sh[3][w][lane] = vmax;
    __syncthreads();
    // qs.stats.max_drawdown: min_t (V_t / max_{s<=t} V_s - 1), the peak seeded by
    // every earlier segment
    double peak = -INFINITY;
    for (int j = 0; j < w; ++j) peak = fmax(peak, sh[3][j][lane]);
    double mdd = 0.0;
    for (t = v0; t < v1; ++t) {
        const double v = values[(size_t)t * B + bb];
        peak = fmax(peak, v);
        mdd = fmin(mdd, v / peak - 1.0);
    }
    sh[4][w][lane] = mdd;
    __syncthreads();
    if (w != 0 || !ok) return;
    double S1 = 0.0, S2 = 0.0, DN = 0.0, MDD = 0.0;
    for (int j = 0; j < 4; ++j) {
        S1 += sh[0][j][lane];
        S2 += sh[1][j][lane];
        DN += sh[2][j][lane];
        MDD = fmin(MDD, sh[4][j][lane]);
    }
    const double mean = K + S1 / T;
    const double sd = T > 1 ? sqrt(fmax(S2 - S1 * S1 / T, 0.0) / (T - 1)) : NAN;
    out[(size_t)b * 5 + 0] = mean / sd * sqrt(periods);
    out[(size_t)b * 5 + 1] = mean / sqrt(DN / T) * sqrt(periods);
    out[(size_t)b * 5 + 2] = MDD;
    out[(size_t)b * 5 + 4] = values[(size_t)T * B + b];
}


// util/eval.py:32-37 average turnover, element-parallel: a workgroup owns `eb` whole
// envs (N <= 256: one thread per (env, asset), so each day's read is eb*N contiguous
// floats) and every thread walks the days keeping the previous weight in a
// register; the env's assets are then summed in a fixed order. N > 256: one env
// per workgroup, threads stride over the assets.
__device__ __forceinline__ void metrics_turnover_body(const float* weights, int T, int B, int N, int tpe, int eb,
                                                      double* out, int bid) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const int el = tid % tpe, le = tid / tpe;
    const int b = bid * eb + le;
    double acc = 0.0;
    if (le < eb && b < B) {
        for (int n = el; n < N; n += tpe) {
            const float* w = weights + (size_t)b * N + n;
            const size_t step = (size_t)B * N;
            float prev = w[0];
            int t = 1;
            for (; t + 3 <= T; t += 4) {
                const float x1 = w[(size_t)t * step], x2 = w[(size_t)(t + 1) * step];
                const float x3 = w[(size_t)(t + 2) * step], x4 = w[(size_t)(t + 3) * step];
                acc += fabs((double)x1 - (double)prev) + fabs((double)x2 - (double)x1) +
                       fabs((double)x3 - (double)x2) + fabs((double)x4 - (double)x3);
                prev = x4;
            }
            for (; t <= T; ++t) {
                const float x = w[(size_t)t * step];
                acc += fabs((double)x - (double)prev);
                prev = x;
            }
        }
    }
    sh[tid] = acc;
    __syncthreads();
    if (el == 0 && le < eb && b < B) {
        double tot = 0.0;
        for (int i = 0; i < tpe; ++i) tot += sh[le * tpe + i];
        out[(size_t)b * 5 + 3] = tot / T;
    }
}


// Both metric passes in one launch: they read disjoint inputs and write disjoint
// fields of out, so the latency-bound segment walk (returns, values) runs beside the
// bandwidth-bound turnover stream (weights) instead of before it. Blocks [0, nseg)
// take the segment walk when seg_first, else the turnover blocks come first.
static __global__ __launch_bounds__(256) void metrics_fused_kernel(const double* returns, const double* values,
                                                            const float* weights, int T, int B, int N, double rf,
                                                            double periods, int tpe, int eb, int nseg, int nturn,
                                                            int seg_first, double* out) {
    const int bid = (int)blockIdx.x;
    const bool seg = seg_first ? bid < nseg : bid >= nturn;
    if (seg) metrics_seg_body(returns, values, T, B, rf, periods, out, seg_first ? bid : bid - nturn);
    else metrics_turnover_body(weights, T, B, N, tpe, eb, out, seg_first ? bid - nseg : bid);
}

// replay/buffer.py:53-79, one workgroup per sample: the W+1 days the pair (s, s')
// spans — market channels from the series, channel F-1 from the recorded actions —
// are staged in LDS as [N][W+1][F], then s (days 0..W-1) and s' (days 1..W) are
// written as whole 16-B chunks when the sample block is 16-B granular.
static __global__ __launch_bounds__(256) void replay_gather_lds_kernel(const float* series, int T, int N, int F, int W,
                                                                const int32_t* days, const float* actions,
                                                                const float* rewards, int H, int B,
                                                                const int32_t* h0, const int32_t* env, float* s,
                                                                float* s_next, float* a_out, float* r_out) {
    extern __shared__ __attribute__((aligned(16))) float ext[];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int b = env[j], hj = h0[j];
    const int Fm = F - 1, W1 = W + 1;
    const int dlast = days[(size_t)((hj + W - 1) % H) * B + b];
    for (int it = tid; it < N * W1; it += 256) {                 // t-major: a day's assets are contiguous
        const int t = it / N, n = it - t * N;
        const int d = dlast - (W - 1) + t;
        float* dst = ext + ((size_t)n * W1 + t) * F;
        const bool in = d >= 0 && d < T;
        const float* src = series + ((size_t)(in ? d : 0) * N + n) * Fm;
        for (int f = 0; f < Fm; ++f) dst[f] = in ? src[f] : NAN;
        dst[Fm] = actions[((size_t)((hj + t) % H) * B + b) * N + n];
    }
    if (tid < N) a_out[(size_t)j * N + tid] = actions[((size_t)((hj + W) % H) * B + b) * N + tid];
    if (tid == 0) r_out[j] = rewards[(size_t)((hj + W - 1) % H) * B + b];
    __syncthreads();
    const int WF = W * F, per = N * WF;
    float* so = s + (size_t)j * per;
    float* sn = s_next + (size_t)j * per;
    if ((per & 3) == 0) {
        for (int q = tid; q < per / 4; q += 256) {
            float v0[4], v1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = 4 * q + k;
                const int n = e / WF, rem = e - n * WF;
                const float* x = ext + (size_t)n * W1 * F + rem;
                v0[k] = x[0];
                v1[k] = x[F];
            }
            reinterpret_cast<f4*>(so)[q] = f4{v0[0], v0[1], v0[2], v0[3]};
            reinterpret_cast<f4*>(sn)[q] = f4{v1[0], v1[1], v1[2], v1[3]};
        }
    } else {
        for (int e = tid; e < per; e += 256) {
            const int n = e / WF, rem = e - n * WF;
            const float* x = ext + (size_t)n * W1 * F + rem;
            so[e] = x[0];
            sn[e] = x[F];
        }
    }
}

// F = 5 form of the LDS gather with every load in flight before the first LDS
// write. Workgroup (j, g) stages sample j's assets [g*R, (g+1)*R) — a few asset
// rows, so the LDS image is ~10 KiB and many workgroups share a CU — thread i
// taking the (day, asset) pairs i, i + 256, ... (PPT at most): the pair's four
// market floats as ONE 16-B load from the [T, N, 4] series and its action as one
// dword; then the image [R][W+1][5] in LDS; then its rows of s and s' as whole
// 16-B chunks (R*W*5 is a multiple of 4, so every group starts 16-B aligned).
// Index divisions by R and W*F are multiply-high.
// NT: cache policy of the s / s' stores (written once, read by the learner later:
// 0 default, 2 nt); TPB threads per workgroup.
template <int PPT, int NT = 0, int TPB = 256>
__global__ __launch_bounds__(TPB) void replay_gather_f5_kernel(const float* series, int T, int N, int W,
                                                               const int32_t* days, const float* actions,
                                                               const float* rewards, int H, int B,
                                                               const int32_t* h0, const int32_t* env, float* s,
                                                               float* s_next, float* a_out, float* r_out, int R,
                                                               FastDiv div_r, FastDiv div_wf) {
    constexpr int F = 5;
    extern __shared__ __attribute__((aligned(16))) float ext[];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int n0 = blockIdx.y * R;
    const int b = env[j], hj = h0[j];
    const int W1 = W + 1;
    // the day index goes out first, the actions (which need only b and hj) behind it,
    // so the wait for the day leaves the action loads in flight
    const int dlast = days[(size_t)((hj + W - 1) % H) * B + b];
    const int P = R * W1;
    f4 mk[PPT];
    float ac[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int it = min(tid + k * TPB, P - 1);
        const int t = (int)fdiv((uint32_t)it, div_r), n = n0 + it - t * R;
        int h = hj + t;
        h = h >= H ? h - H : h;
        ac[k] = actions[((size_t)h * B + b) * N + n];
    }
    const int d0 = dlast - (W - 1);
    const auto rs_ser = make_rsrc(series, (uint32_t)T * (uint32_t)N * 16u);
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int it = min(tid + k * TPB, P - 1);
        const int t = (int)fdiv((uint32_t)it, div_r), n = n0 + it - t * R;
        const int d = d0 + t;
        const bool in = tid + k * TPB < P && d >= 0 && d < T;   // days off the series read NaN below
        mk[k] = buf_load4(rs_ser, in ? ((uint32_t)d * (uint32_t)N + (uint32_t)n) * 16u : 0xFFFFFFF0u);
    }
    if (tid < R) a_out[(size_t)j * N + n0 + tid] = actions[((size_t)((hj + W) % H) * B + b) * N + n0 + tid];
    if (tid == 0 && blockIdx.y == 0) r_out[j] = rewards[(size_t)((hj + W - 1) % H) * B + b];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int it = tid + k * TPB;
        if (it < P) {
            const int t = (int)fdiv((uint32_t)it, div_r), nl = it - t * R;
            const int d = d0 + t;
            const bool in = d >= 0 && d < T;
            float* dst = ext + ((size_t)nl * W1 + t) * F;
            dst[0] = in ? mk[k].x : NAN;
            dst[1] = in ? mk[k].y : NAN;
            dst[2] = in ? mk[k].z : NAN;
            dst[3] = in ? mk[k].w : NAN;
            dst[4] = ac[k];
        }
    }
    __syncthreads();
    const int WF = W * F, per = R * WF;
    float* so = s + (size_t)j * N * WF + (size_t)n0 * WF;
    float* sn = s_next + (size_t)j * N * WF + (size_t)n0 * WF;
    const auto rso = make_rsrc(so, (uint32_t)per * 4u), rsn = make_rsrc(sn, (uint32_t)per * 4u);
    for (int q = tid; q < per / 4; q += TPB) {
        float v0[4], v1[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = 4 * q + k;
            const int n = (int)fdiv((uint32_t)e, div_wf);
            const float* x = ext + (size_t)n * F + e;       // LDS row n starts n*F floats later than in s
            v0[k] = x[0];
            v1[k] = x[F];
        }
        buf_store4<NT>(rso, (uint32_t)q * 16u, f4{v0[0], v0[1], v0[2], v0[3]});
        buf_store4<NT>(rsn, (uint32_t)q * 16u, f4{v1[0], v1[1], v1[2], v1[3]});
    }
}


// The F = 5 gather as a persistent loop: workgroup g takes samples g, g + G, g + 2G, ..
// and keeps the pipeline full across them — the next sample's staging loads go out
// (into the same registers, once the current image is in LDS) before the current
// sample's write-out, and its index chain (env / h0, then the day) is fetched two and
// one samples ahead — so a sample costs its write-out, not three dependent memory
// round trips plus the write-out. Same image and write-out as replay_gather_f5_kernel.
template <int PPT, int NT>
__global__ __launch_bounds__(256) void replay_gather_f5p_kernel(const float* series, int T, int N, int W,
                                                                const int32_t* days, const float* actions,
                                                                const float* rewards, int H, int B,
                                                                const int32_t* h0, const int32_t* env, int S, float* s,
                                                                float* s_next, float* a_out, float* r_out, int R,
                                                                FastDiv div_r, FastDiv div_wf) {
    constexpr int F = 5;
    extern __shared__ __attribute__((aligned(16))) float ext[];
    const int tid = threadIdx.x;
    const int n0 = blockIdx.y * R;
    const int W1 = W + 1, P = R * W1, WF = W * F, per = R * WF;
    const int G = gridDim.x;
    int j = blockIdx.x;
    if (j >= S) return;                                    // uniform per workgroup
    const auto rs_ser = make_rsrc(series, (uint32_t)T * (uint32_t)N * 16u);
    auto day_of = [&](int bb, int hh) { return days[(size_t)((hh + W - 1) % H) * B + bb]; };
    f4 mk[PPT];
    float ac[PPT];
    auto issue = [&](int bb, int hh, int dl) {            // the sample's staging loads, nothing waited
        const int d0 = dl - (W - 1);
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int it = min(tid + k * 256, P - 1);
            const int t = (int)fdiv((uint32_t)it, div_r), n = n0 + it - t * R;
            int h = hh + t;
            h = h >= H ? h - H : h;
            ac[k] = actions[((size_t)h * B + bb) * N + n];
            const int d = d0 + t;
            const bool in = tid + k * 256 < P && d >= 0 && d < T;
            mk[k] = buf_load4(rs_ser, in ? ((uint32_t)d * (uint32_t)N + (uint32_t)n) * 16u : 0xFFFFFFF0u);
        }
    };
    // index pipeline: (b0, h0, d0) current; (b1, h1, d1) next; (b2, h2) the one after
    int bc = env[j], hc = h0[j];
    int dc = day_of(bc, hc);
    bool m1 = j + G < S, m2 = j + 2 * G < S;
    int b1 = 0, h1 = 0, d1 = 0, b2 = 0, h2 = 0;
    if (m1) { b1 = env[j + G]; h1 = h0[j + G]; }
    if (m2) { b2 = env[j + 2 * G]; h2 = h0[j + 2 * G]; }
    if (m1) d1 = day_of(b1, h1);
    issue(bc, hc, dc);
    while (true) {
        if (tid < R) a_out[(size_t)j * N + n0 + tid] = actions[((size_t)((hc + W) % H) * B + bc) * N + n0 + tid];
        if (tid == 0 && blockIdx.y == 0) r_out[j] = rewards[(size_t)((hc + W - 1) % H) * B + bc];
        const int dfirst = dc - (W - 1);
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int it = tid + k * 256;
            if (it < P) {
                const int t = (int)fdiv((uint32_t)it, div_r), nl = it - t * R;
                const int d = dfirst + t;
                const bool in = d >= 0 && d < T;
                float* dst = ext + ((size_t)nl * W1 + t) * F;
                dst[0] = in ? mk[k].x : NAN;
                dst[1] = in ? mk[k].y : NAN;
                dst[2] = in ? mk[k].z : NAN;
                dst[3] = in ? mk[k].w : NAN;
                dst[4] = ac[k];
            }
        }
        __syncthreads();
        if (m1) issue(b1, h1, d1);                          // the next sample's loads fly during the write-out
        float* so = s + (size_t)j * N * WF + (size_t)n0 * WF;
        float* sn = s_next + (size_t)j * N * WF + (size_t)n0 * WF;
        const auto rso = make_rsrc(so, (uint32_t)per * 4u), rsn = make_rsrc(sn, (uint32_t)per * 4u);
        for (int q = tid; q < per / 4; q += 256) {
            float v0[4], v1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = 4 * q + k;
                const int n = (int)fdiv((uint32_t)e, div_wf);
                const float* x = ext + (size_t)n * F + e;
                v0[k] = x[0];
                v1[k] = x[F];
            }
            buf_store4<NT>(rso, (uint32_t)q * 16u, f4{v0[0], v0[1], v0[2], v0[3]});
            buf_store4<NT>(rsn, (uint32_t)q * 16u, f4{v1[0], v1[1], v1[2], v1[3]});
        }
        // index chain ahead: the day of the sample after next, env / h0 of the one after that
        const int j3 = j + 3 * G;
        const bool m3 = j3 < S;
        const int d2 = m2 ? day_of(b2, h2) : 0;
        int b3 = 0, h3 = 0;
        if (m3) { b3 = env[j3]; h3 = h0[j3]; }
        __syncthreads();                                   // the image is rewritten next
        if (!m1) break;
        j += G;
        bc = b1; hc = h1; dc = d1;
        b1 = b2; h1 = h2; d1 = d2; m1 = m2;
        b2 = b3; h2 = h3; m2 = m3;
    }
}

// ---------------------------------------------------------------- n-step samples
// agent/td3/td3.py:85-106 (add_experience) folds the last n_step transitions into one
// before it stores them: reward = r + gamma * reward * (1 - d) from the back (:94-96),
// the first state and action, the next state of the step where the fold stopped. Here
// the ring already holds every step, so the fold happens at sample time: for a valid
// one-step sample (h0, b), with st = (h0 - oldest) mod H its position in the ring,
//   m  = the largest count in [1, n] whose one-step starts st .. st+m-1 are all valid:
//        st+m-1 < count-W-1 and rows st .. st+m-1+W share one episode (td3's `done`:
//        an episode boundary or the newest recorded rows end the fold early)
//   s, a = the one-step sample's at h0;  s' = the one-step sample's s' at h0+m-1
//   R  = sum_{k<m} gamma^k rewards[h0+W-1+k, b], Horner from the last term in f64
//   steps = m, discount = gamma^m (f64 product)
// Episode ids do not decrease from the oldest row to the newest, so the rows
// st .. st+k+W share one episode iff the last one carries the first one's id.

struct NstepRing {
    const int32_t* row_ep;   // episode id of ring row h for env b at [h * stride_h + b * stride_b], nullptr = one episode
    int oldest, count, n;
    double gamma;
    int stride_h, stride_b;  // (1, 0): one id per row [H], the envs in lockstep; (B, 1): one per (row, env) [H, B]
};
// How a kernel addresses the ids. The f5p kernels are built once per layout — the lockstep
// instantiation reads ids[h], the code it had before there was a second layout, and the
// *_env_kernel one reads ids[h * B + b] — because the runtime strides cost the lockstep
// gathers 1-3 % at config 3; the other forms take the strides.
enum { kEpRow = 0, kEpEnv = 1, kEpStrided = 2 };
template <int MODE = kEpStrided>
__device__ __forceinline__ int ring_ep(const NstepRing& rg, const int32_t* __restrict__ ids, int h, int b) {
    if constexpr (MODE == kEpRow) return ids[h];
    // one 32 x 32 -> 64-bit multiply-add (stride_b is 0 or 1: b * stride_b < B)
    if constexpr (MODE == kEpEnv) return ids[(uint64_t)(uint32_t)h * (uint32_t)rg.stride_h + (uint32_t)b];
    return ids[(uint64_t)(uint32_t)h * (uint32_t)rg.stride_h + (uint32_t)b * (uint32_t)rg.stride_b];
}

// the cap nn of m from the recorded rows alone, and the episode ids that decide
// whether it holds: E of row h, far of the last row of start st+nn-1
__device__ __forceinline__ int nstep_cap(const NstepRing& rg, int H, int W, int h) {
    int st = h - rg.oldest;
    st = st < 0 ? st + H : st;
    const int nn = min(rg.n, rg.count - W - 1 - st);
    return nn < 1 ? 1 : nn;
}
// ring rows below 2H / 3H back into [0, H) without a division
__device__ __forceinline__ int ring_wrap(int x, int H) { return x >= H ? x - H : x; }
__device__ __forceinline__ int nstep_last_row(int H, int W, int h, int k) {   // k <= count - W - 1
    return ring_wrap(ring_wrap(h + W + k - 1, H), H);
}
// m from E, far: nn when the farthest window still lies in the episode (two loads, one
// round trip), else the boundary by bisection — start st is valid, start st+nn-1 is not
template <int MODE = kEpStrided>
__device__ __forceinline__ int nstep_finish(const NstepRing& rg, int H, int W, int h, int b, int nn, int E,
                                            int far) {
    if (far == E) return nn;
    int lo = 1, hi = nn;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ring_ep<MODE>(rg, rg.row_ep, nstep_last_row(H, W, h, mid), b) == E) lo = mid;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int nstep_count(const NstepRing& rg, int H, int W, int h, int b) {
    const int nn = nstep_cap(rg, H, W, h);
    if (!rg.row_ep || nn == 1) return nn;
    return nstep_finish(rg, H, W, h, b, nn, ring_ep(rg, rg.row_ep, h, b),
                        ring_ep(rg, rg.row_ep, nstep_last_row(H, W, h, nn), b));
}

// R and gamma^m by one thread: acc = r_k + gamma * acc from the last term (td3.py:94-96)
__device__ __forceinline__ void nstep_fold_serial(const float* rewards, int H, int B, int b, int hr, int m,
                                                  double gamma, float* R, float* disc) {
    double acc = 0.0, g = 1.0;
    for (int k = m - 1; k >= 0; --k) {
        acc = (double)rewards[(size_t)((hr + k) % H) * B + b] + gamma * acc;
        g *= gamma;
    }
    *R = (float)acc;
    *disc = (float)g;
}

// The same fold by one wave: lane l holds reward k0 + l of a chunk of 64 (`first` is the
// chunk k0 = 0, loaded with the sample's staging loads), the Horner chain walks the
// lanes from the back through v_readlane — the m loads are not a dependent chain.
__device__ __forceinline__ void nstep_fold_wave(const float* rewards, int H, int B, int b, int hr, int m, float first,
                                                double gamma, float* R, float* disc) {
    const int lane = threadIdx.x & 63;
    double acc = 0.0, g = 1.0;
    for (int k0 = ((m - 1) >> 6) << 6; k0 >= 0; k0 -= 64) {
        float r = first;
        if (k0 > 0) r = rewards[(size_t)((hr + min(k0 + lane, m - 1)) % H) * B + b];
        // at least one term a chunk: the loaded chunk is always consumed here, so no load
        // of the fold is still in flight (as far as the compiler can tell) after it
        int l = min(64, m - k0) - 1;
        do {
            const float rl = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(r), l));
            acc = (double)rl + gamma * acc;
            g *= gamma;
        } while (--l >= 0);
    }
    if (lane == 0) {
        *R = (float)acc;
        *disc = (float)g;
    }
}

// one thread per output float of s and s' (the last resort: any F, N and alignment);
// a / R / steps / discount by the first threads. Every thread finds its sample's m.
static __global__ void replay_nstep_kernel(const float* series, int T, int N, int F, int W, const int32_t* days,
                                           const float* actions, const float* rewards, int H, int B,
                                           const int32_t* h0, const int32_t* env, int S, NstepRing rg, float* s,
                                           float* s_next, float* a_out, float* r_out, int32_t* steps,
                                           float* discount) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per = (int64_t)N * W * F;
    const int Fm = F - 1;
    if (i < (int64_t)S * N) {                     // a = actions[h0+W]; the fold by the sample's first thread
        const int j = (int)(i / N), n = (int)(i % N);
        const int b = env[j];
        const int ha = (h0[j] + W) % H;
        a_out[i] = actions[((size_t)ha * B + b) * N + n];
        if (n == 0) {
            const int m = nstep_count(rg, H, W, h0[j], b);
            steps[j] = m;
            nstep_fold_serial(rewards, H, B, b, (h0[j] + W - 1) % H, m, rg.gamma, r_out + j, discount + j);
        }
    }
    if (i >= (int64_t)S * per) return;
    const int j = (int)(i / per);
    int rem = (int)(i - (int64_t)j * per);
    const int n = rem / (W * F);
    rem -= n * W * F;
    const int t = rem / F, f = rem - t * F;
    const int b = env[j], hj = h0[j];
    const int m = nstep_count(rg, H, W, hj, b);
    float v, vn;
    if (f < Fm) {
        const int d = days[(size_t)((hj + W - 1) % H) * B + b] - (W - 1) + t;           // s: the window of h0
        const int dn = days[(size_t)((hj + m + W - 2) % H) * B + b] + 1 - (W - 1) + t;  // s': one past h0+m-1's
        v = (d >= 0 && d < T) ? series[((size_t)d * N + n) * Fm + f] : NAN;
        vn = (dn >= 0 && dn < T) ? series[((size_t)dn * N + n) * Fm + f] : NAN;
    } else {
        v = actions[((size_t)((hj + t) % H) * B + b) * N + n];
        vn = actions[((size_t)((hj + m + t) % H) * B + b) * N + n];
    }
    s[i] = v;
    s_next[i] = vn;
}

// One workgroup per sample, any F: the days the pair spans are staged in LDS as
// [N][D][F] (D = W + min(n, W) rows reserved). Where s' starts m <= W days after s the
// two windows are one image of W + m days, every series line and action row fetched
// once; otherwise (disjoint windows, or day indices that do not advance by one a row)
// the image holds s, then s', in two passes.
static __global__ __launch_bounds__(256) void replay_nstep_lds_kernel(const float* series, int T, int N, int F, int W,
                                                               const int32_t* days, const float* actions,
                                                               const float* rewards, int H, int B,
                                                               const int32_t* h0, const int32_t* env, NstepRing rg,
                                                               int D, float* s, float* s_next, float* a_out,
                                                               float* r_out, int32_t* steps, float* discount) {
    extern __shared__ __attribute__((aligned(16))) float ext[];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int b = env[j], hj = h0[j];
    const int Fm = F - 1;
    const int m = nstep_count(rg, H, W, hj, b);                     // uniform: one sample per workgroup
    const float rw = tid < min(m, 64) ? rewards[(size_t)((hj + W - 1 + tid) % H) * B + b] : 0.0f;
    const int dA = days[(size_t)((hj + W - 1) % H) * B + b] - (W - 1);
    const int dB = days[(size_t)((hj + m + W - 2) % H) * B + b] + 1 - (W - 1);
    const bool joint = dB - dA == m && m <= D - W;
    const int WF = W * F, per = N * WF;
    float* so = s + (size_t)j * per;
    float* sn = s_next + (size_t)j * per;
    const bool vec = (per & 3) == 0;
    auto stage = [&](int hA, int d0, int nd) {                   // t-major: a day's assets are contiguous
        for (int it = tid; it < N * nd; it += 256) {
            const int t = it / N, n = it - t * N;
            const int d = d0 + t;
            float* dst = ext + ((size_t)n * D + t) * F;
            const bool in = d >= 0 && d < T;
            const float* src = series + ((size_t)(in ? d : 0) * N + n) * Fm;
            for (int f = 0; f < Fm; ++f) dst[f] = in ? src[f] : NAN;
            dst[Fm] = actions[((size_t)((hA + t) % H) * B + b) * N + n];
        }
    };
    auto emit = [&](float* out, int day0) {                      // image days day0 .. day0+W-1 -> [N, W, F]
        if (vec) {
            for (int q = tid; q < per / 4; q += 256) {
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = 4 * q + k;
                    const int n = e / WF, rem = e - n * WF;
                    v[k] = ext[((size_t)n * D + day0) * F + rem];
                }
                reinterpret_cast<f4*>(out)[q] = f4{v[0], v[1], v[2], v[3]};
            }
        } else {
            for (int e = tid; e < per; e += 256) {
                const int n = e / WF, rem = e - n * WF;
                out[e] = ext[((size_t)n * D + day0) * F + rem];
            }
        }
    };
    if (tid < N) a_out[(size_t)j * N + tid] = actions[((size_t)((hj + W) % H) * B + b) * N + tid];
    if (joint) {
        stage(hj, dA, W + m);
        __syncthreads();
        emit(so, 0);
        emit(sn, m);
    } else {
        stage(hj, dA, W);
        __syncthreads();
        emit(so, 0);
        __syncthreads();
        stage((hj + m) % H, dB, W);
        __syncthreads();
        emit(sn, 0);
    }
    if (tid < 64) {
        if (tid == 0) steps[j] = m;
        nstep_fold_wave(rewards, H, B, b, (hj + W - 1) % H, m, rw, rg.gamma, r_out + j, discount + j);
    }
}

// The F = 5 n-step gather, persistent like replay_gather_f5p_kernel: workgroup g takes
// samples g, g + G, .. and runs them as a sequence of passes over one LDS image
// [R][D][5] (D = W + min(n, W)):
//   joint  (s' starts m <= W days after s): W + m days staged once, s from day 0, s' from day m
//   first / second (disjoint windows, or days that do not advance by one a row): s, then s'
// The next pass's staging loads — market float4s, actions and, for a sample's first
// pass, its first 64 rewards in wave 0 — go out once the current image is in LDS, before
// the write-out; wave 0 folds the current sample's rewards just before it issues them. The index chain runs three samples ahead, one memory level a sample:
// env / h0, then the day of s with the two episode ids that decide m, then the day of s'.
template <int PPT, int NT, int MODE>
__device__ __forceinline__ void replay_nstep_f5p_body(const float* __restrict__ series, int T, int N, int W,
                                                      const int32_t* __restrict__ days,
                                                      const float* __restrict__ actions,
                                                      const float* __restrict__ rewards, int H, int B,
                                                      const int32_t* __restrict__ h0,
                                                      const int32_t* __restrict__ env, int S, NstepRing rg, int D,
                                                      float* s, float* s_next, float* a_out, float* r_out,
                                                      int32_t* steps, float* discount, int R, FastDiv div_r,
                                                      FastDiv div_wf) {
    constexpr int F = 5;
    extern __shared__ __attribute__((aligned(16))) float ext[];
    const int tid = threadIdx.x;
    const int n0 = blockIdx.y * R;
    const int WF = W * F, per = R * WF;
    const int G = gridDim.x;
    int j = blockIdx.x;
    if (j >= S) return;                                    // uniform per workgroup
    const auto rs_ser = make_rsrc(series, (uint32_t)T * (uint32_t)N * 16u);
    const bool folds = tid < 64 && blockIdx.y == 0;        // wave 0 of the sample's first asset group
    f4 mk[PPT];
    float ac[PPT];
    float rw = 0.0f;
    // the staging loads of one pass, nothing waited: nd days from day d0 and ring row hA;
    // mr > 0: the pass opens a sample of mr steps whose rewards start at row hr
    // (a lane past the pass's pairs repeats the last pair's action load, as the one-step
    // kernel does: a select on the loaded value would wait for every load in turn)
    auto issue = [&](int bb, int hA, int d0, int nd, int mr, int hr) {
        if (folds && mr > 0) rw = rewards[(size_t)ring_wrap(hr + min(tid, mr - 1), H) * B + bb];
        const int P = R * nd;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int it = min(tid + k * 256, P - 1);
            const int t = (int)fdiv((uint32_t)it, div_r), n = n0 + it - t * R;
            const int h = ring_wrap(hA + t, H);            // t < W + m <= H - 1
            ac[k] = actions[((size_t)h * B + bb) * N + n];
            const int d = d0 + t;
            const bool in = tid + k * 256 < P && d >= 0 && d < T;
            mk[k] = buf_load4(rs_ser, in ? ((uint32_t)d * (uint32_t)N + (uint32_t)n) * 16u : 0xFFFFFFF0u);
        }
    };
    // rows below 2H; a NULL row_episode reads the day array instead and ignores the ids
    auto day_at = [&](int bb, int row) { return days[(size_t)ring_wrap(row, H) * B + bb]; };
    const bool has_ep = rg.row_ep != nullptr;
    const int32_t* __restrict__ epp = has_ep ? rg.row_ep : days;
    // index pipeline. c: the sample in hand, 1: the next (complete: b, h, m, dA, dB),
    // 2: b, h, cap, the ids E / far and dA loaded (m follows without a load unless an
    // episode ends inside the cap), 3: b, h
    int bc, hc, mc, dAc, dBc;
    int b1 = 0, h1 = 0, m1 = 1, dA1 = 0, dB1 = 0;
    int b2 = 0, h2 = 0, nn2 = 1, E2 = 0, far2 = 0, dA2 = 0;
    int b3 = 0, h3 = 0;
    bool v1 = j + G < S, v2 = j + 2 * G < S, v3 = j + 3 * G < S;
    auto level2 = [&](int bb, int hh, int& nn, int& E, int& far, int& dA) {    // three loads, no branch
        nn = nstep_cap(rg, H, W, hh);
        E = ring_ep<MODE>(rg, epp, hh, bb);
        far = ring_ep<MODE>(rg, epp, nstep_last_row(H, W, hh, nn), bb);
        dA = day_at(bb, hh + W - 1) - (W - 1);
    };
    auto finish = [&](int bb, int hh, int nn, int E, int far) {
        return has_ep ? nstep_finish<MODE>(rg, H, W, hh, bb, nn, E, far) : nn;
    };
    auto level3 = [&](int bb, int hh, int mm) { return day_at(bb, hh + mm + W - 2) + 1 - (W - 1); };
    bc = env[j]; hc = h0[j];
    if (v1) { b1 = env[j + G]; h1 = h0[j + G]; }
    if (v2) { b2 = env[j + 2 * G]; h2 = h0[j + 2 * G]; }
    if (v3) { b3 = env[j + 3 * G]; h3 = h0[j + 3 * G]; }
    {
        int nn, E, far;
        level2(bc, hc, nn, E, far, dAc);
        mc = finish(bc, hc, nn, E, far);
        dBc = level3(bc, hc, mc);
        if (v1) {
            level2(b1, h1, nn, E, far, dA1);
            m1 = finish(b1, h1, nn, E, far);
            dB1 = level3(b1, h1, m1);
        }
        if (v2) level2(b2, h2, nn2, E2, far2, dA2);
    }
    bool joint = dBc - dAc == mc && mc <= D - W;
    int pass = joint ? 0 : 1;                              // 0 joint, 1 first (s), 2 second (s')
    issue(bc, hc, dAc, joint ? W + mc : W, mc, ring_wrap(hc + W - 1, H));
    while (true) {
        const int nd = pass == 0 ? W + mc : W;
        const int dfirst = pass == 2 ? dBc : dAc;
        if (pass != 2 && tid < R)
            a_out[(size_t)j * N + n0 + tid] = actions[((size_t)ring_wrap(hc + W, H) * B + bc) * N + n0 + tid];
        const int P = R * nd;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int it = tid + k * 256;
            if (it < P) {
                const int t = (int)fdiv((uint32_t)it, div_r), nl = it - t * R;
                const int d = dfirst + t;
                const bool in = d >= 0 && d < T;
                float* dst = ext + ((size_t)nl * D + t) * F;
                dst[0] = in ? mk[k].x : NAN;
                dst[1] = in ? mk[k].y : NAN;
                dst[2] = in ? mk[k].z : NAN;
                dst[3] = in ? mk[k].w : NAN;
                dst[4] = ac[k];
            }
        }
        __syncthreads();
        // the fold sits here, where nothing this wave waits for is in flight but the last
        // write-out's stores: behind the next pass's loads its waits would be theirs.
        // Wave 0 then issues its share of them late, with the whole write-out to land in
        if (pass != 2 && folds) {
            if (tid == 0) steps[j] = mc;
            nstep_fold_wave(rewards, H, B, bc, ring_wrap(hc + W - 1, H), mc, rw, rg.gamma, r_out + j, discount + j);
        }
        // the next pass's loads fly during the write-out
        const bool last_of_sample = pass != 1;
        if (pass == 1) {
            issue(bc, ring_wrap(hc + mc, H), dBc, W, 0, 0);
        } else if (v1) {
            const bool jn = dB1 - dA1 == m1 && m1 <= D - W;
            issue(b1, h1, dA1, jn ? W + m1 : W, m1, ring_wrap(h1 + W - 1, H));
        }
        float* so = s + (size_t)j * N * WF + (size_t)n0 * WF;
        float* sn = s_next + (size_t)j * N * WF + (size_t)n0 * WF;
        const auto rso = make_rsrc(so, (uint32_t)per * 4u), rsn = make_rsrc(sn, (uint32_t)per * 4u);
        const int skip = (D - W) * F;                      // LDS row n starts n*skip floats later than in s
        if (pass == 0) {
            const int off = mc * F;
            for (int q = tid; q < per / 4; q += 256) {
                float v0[4], vn[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = 4 * q + k;
                    const int n = (int)fdiv((uint32_t)e, div_wf);
                    const float* x = ext + (__umul24(n, skip) + e);   // 24-bit multiply: full rate
                    v0[k] = x[0];
                    vn[k] = x[off];
                }
                buf_store4<NT>(rso, (uint32_t)q * 16u, f4{v0[0], v0[1], v0[2], v0[3]});
                buf_store4<NT>(rsn, (uint32_t)q * 16u, f4{vn[0], vn[1], vn[2], vn[3]});
            }
        } else {
            const auto rs_out = pass == 1 ? rso : rsn;
            for (int q = tid; q < per / 4; q += 256) {
                float v0[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = 4 * q + k;
                    const int n = (int)fdiv((uint32_t)e, div_wf);
                    v0[k] = ext[__umul24(n, skip) + e];
                }
                buf_store4<NT>(rs_out, (uint32_t)q * 16u, f4{v0[0], v0[1], v0[2], v0[3]});
            }
        }
        if (!last_of_sample) {
            __syncthreads();                               // the image is rewritten next
            pass = 2;
            continue;
        }
        // index chain ahead, one level each: sample 2 completes (its ids and dA were
        // loaded a sample ago), sample 3 loads its ids and dA, sample 4 its env / h0. Six
        // loads in one block without a branch (a slot past S holds row 0 of env 0), so one
        // round trip covers them
        const int j4 = j + 4 * G;
        const bool v4 = j4 < S;
        const int m2 = finish(b2, h2, nn2, E2, far2);
        const int dB2 = level3(b2, h2, m2);
        int nn3, E3, far3, dA3;
        level2(b3, h3, nn3, E3, far3, dA3);
        const int b4 = env[min(j4, S - 1)], h4 = h0[min(j4, S - 1)];
        __syncthreads();                                   // the image is rewritten next
        if (!v1) break;
        j += G;
        bc = b1; hc = h1; mc = m1; dAc = dA1; dBc = dB1;
        b1 = b2; h1 = h2; m1 = m2; dA1 = dA2; dB1 = dB2; v1 = v2;
        b2 = b3; h2 = h3; nn2 = nn3; E2 = E3; far2 = far3; dA2 = dA3; v2 = v3;
        b3 = b4; h3 = h4; v3 = v4;
        pass = (dBc - dAc == mc && mc <= D - W) ? 0 : 1;
    }
}

#define PMENV_NSTEP_F5P_ARGS                                                                                         \
    const float *__restrict__ series, int T, int N, int W, const int32_t *__restrict__ days,                        \
        const float *__restrict__ actions, const float *__restrict__ rewards, int H, int B,                         \
        const int32_t *__restrict__ h0, const int32_t *__restrict__ env, int S, NstepRing rg, int D, float *s,      \
        float *s_next, float *a_out, float *r_out, int32_t *steps, float *discount, int R, FastDiv div_r,           \
        FastDiv div_wf
// one id per ring row (rg.row_ep [H], or nullptr)
template <int PPT, int NT>
__global__ __launch_bounds__(256) void replay_nstep_f5p_kernel(PMENV_NSTEP_F5P_ARGS) {
    replay_nstep_f5p_body<PPT, NT, kEpRow>(series, T, N, W, days, actions, rewards, H, B, h0, env, S, rg, D, s,
                                           s_next, a_out, r_out, steps, discount, R, div_r, div_wf);
}
// one id per (ring row, env) (rg.row_ep [H, B], rg.stride_h = B)
template <int PPT, int NT>
__global__ __launch_bounds__(256) void replay_nstep_f5p_env_kernel(PMENV_NSTEP_F5P_ARGS) {
    replay_nstep_f5p_body<PPT, NT, kEpEnv>(series, T, N, W, days, actions, rewards, H, B, h0, env, S, rg, D, s,
                                           s_next, a_out, r_out, steps, discount, R, div_r, div_wf);
}
#undef PMENV_NSTEP_F5P_ARGS

// ---------------------------------------------------------------- sequence samples
// agent/dreamer/dreamer.py:77-80 trains its world model on sequences of consecutive
// steps (world_model.py:41-64 walks them time-major). Element t of sequence j is the
// one-step sample at start (h0[j] + t) mod H of env[j]: x = its s, a = its a_out, r = its
// r_out. length[j] = m is the n-step count with n = L (NstepRing.n holds L): an episode
// boundary or the newest recorded rows cut a sequence short, and the elements t >= m are
// written as +0.0. e(j, t) = t*S + j (time-major) or j*L + t is the element's slot in
// x [.., N, W, F], a_out [.., N] and r_out [..].

// one thread per output float of x (any F, N and alignment, and rings whose day indices
// skip: every element looks up its own day); a / r / length by the first threads
static __global__ void replay_seq_kernel(const float* series, int T, int N, int F, int W, const int32_t* days,
                                         const float* actions, const float* rewards, int H, int B,
                                         const int32_t* h0, const int32_t* env, int S, NstepRing rg, int time_major,
                                         float* x, float* a_out, float* r_out, int32_t* length) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int L = rg.n, Fm = F - 1;
    const int64_t per = (int64_t)N * W * F;
    auto slot = [&](int64_t e, int& j, int& t) {       // element slot -> (sequence, position)
        if (time_major) { t = (int)(e / S); j = (int)(e - (int64_t)t * S); }
        else { j = (int)(e / L); t = (int)(e - (int64_t)j * L); }
    };
    if (i < (int64_t)S * L * N) {                       // a = actions[h0+t+W], r = rewards[h0+t+W-1]
        const int64_t e = i / N;
        const int n = (int)(i - e * N);
        int j, t;
        slot(e, j, t);
        const int b = env[j], hj = h0[j];
        const int m = nstep_count(rg, H, W, hj, b);
        const bool live = t < m;                        // t < m <= H: the rows below stay under 3H
        a_out[i] = live ? actions[((size_t)ring_wrap(ring_wrap(hj + W + t, H), H) * B + b) * N + n] : 0.0f;
        if (n == 0) {
            r_out[e] = live ? rewards[(size_t)ring_wrap(ring_wrap(hj + W - 1 + t, H), H) * B + b] : 0.0f;
            if (t == 0) length[j] = m;
        }
    }
    if (i >= (int64_t)S * L * per) return;
    const int64_t e = i / per;
    int rem = (int)(i - e * per);
    int j, t;
    slot(e, j, t);
    const int n = rem / (W * F);
    rem -= n * W * F;
    const int p = rem / F, f = rem - p * F;
    const int b = env[j], hj = h0[j];
    float v = 0.0f;
    if (t < nstep_count(rg, H, W, hj, b)) {
        const int ht = ring_wrap(hj + t, H);            // the element's one-step start
        if (f < Fm) {
            const int d = days[(size_t)ring_wrap(ht + W - 1, H) * B + b] - (W - 1) + p;
            v = (d >= 0 && d < T) ? series[((size_t)d * N + n) * Fm + f] : NAN;
        } else {
            v = actions[((size_t)ring_wrap(ht + p, H) * B + b) * N + n];
        }
    }
    x[i] = v;
}

// The F = 5 sequence gather, persistent (one workgroup per CU). A work item is (sequence j,
// asset group g of R rows, chunk c of Lc elements); workgroup w takes items w, w + G, ..
// The item's live elements (cnt = those below m) share ONE LDS image [R][D][5], D = W + Lc:
// W + cnt - 1 series days (16-B loads) and W + cnt action rows, the last row for a_out
// alone. Element t's [R, W, 5] block is the image shifted by t days, i.e. by 5t floats in
// every asset row, so the windows leave as 16-B global stores whose four floats are read
// from LDS one dword each: the shift is 20t bytes, 16-B aligned only for t % 4 == 0, and
// dword reads run at 128 B/clk/CU, far above what one CU's share of the write stream asks.
// The source offsets of a lane's quad are computed once and reused for every element.
// Elements >= m take the same stores with zeros. The next item's staging loads go out once
// the current image is in LDS, before the write-out. Its indices are resolved one item
// earlier still: env / h0 of the item after next are loaded during a write-out, and after
// it the episode ids that give m and the chunk's day indices. A chunk whose days do not
// advance by one a row (a caller's own ring) is staged and written element by element.
// NT: cache-policy bits of the window stores (0 plain, 2 nt, 16 sc1).
template <int PPT, int NT, int MODE>
__device__ __forceinline__ void replay_seq_f5p_body(const float* __restrict__ series, int T, int N, int W,
                                                    const int32_t* __restrict__ days,
                                                    const float* __restrict__ actions,
                                                    const float* __restrict__ rewards, int H, int B,
                                                    const int32_t* __restrict__ h0,
                                                    const int32_t* __restrict__ env, int S, NstepRing rg, int Lc,
                                                    int nc, int time_major, float* x, float* a_out, float* r_out,
                                                    int32_t* length, int R, FastDiv div_r, FastDiv div_wf,
                                                    FastDiv div_nc, FastDiv div_gy) {
    constexpr int F = 5;
    extern __shared__ __attribute__((aligned(16))) float ext[];
    int* flg = reinterpret_cast<int*>(ext);                // [4] each wave's verdict on a chunk's days
    float* img = ext + 4;
    const int tid = threadIdx.x, G = gridDim.x;
    const int L = rg.n, gy = N / R, D = W + Lc;
    const int WF = W * F, per = R * WF, skip = Lc * F;     // LDS row n starts n*skip floats later than in x
    const int items = S * gy * nc;
    if ((int)blockIdx.x >= items) return;                  // uniform per workgroup
    const auto rs_ser = make_rsrc(series, (uint32_t)T * (uint32_t)N * 16u);
    const bool has_ep = rg.row_ep != nullptr;
    const int32_t* __restrict__ epp = has_ep ? rg.row_ep : days;
    // an item: its sequence, group and chunk; env and start; m; the live elements of the
    // chunk; the first staged day; whether the chunk's days advance by one a row
    struct Item {
        int j, n0, t0, b, h, m, cnt, dA, one;
    };
    auto raw = [&](int i, Item& it) {                      // env / h0: the first level of the chain
        const int sg = (int)fdiv((uint32_t)i, div_nc);
        it.j = (int)fdiv((uint32_t)sg, div_gy);
        it.n0 = (sg - it.j * gy) * R;
        it.t0 = (i - sg * nc) * Lc;
        it.b = env[it.j];
        it.h = h0[it.j];
    };
    // the second level: two episode ids, the chunk's first day and this thread's day, one
    // round trip; then a verdict through LDS (two barriers: the image may be rewritten after)
    auto resolve = [&](Item& it) {
        const int nn = nstep_cap(rg, H, W, it.h);          // m <= nn <= count - W - 1 < H
        const int tc = min(it.t0, nn - 1);                 // a chunk past nn is empty: any rows do
        const int span = min(Lc, nn - tc);
        const int row0 = ring_wrap(ring_wrap(it.h + W - 1, H) + tc, H);
        const int E = ring_ep<MODE>(rg, epp, it.h, it.b);
        const int far = ring_ep<MODE>(rg, epp, nstep_last_row(H, W, it.h, nn), it.b);
        const int dfirst = days[(size_t)row0 * B + it.b];
        const int dmine = days[(size_t)ring_wrap(row0 + min(tid, span - 1), H) * B + it.b];
        it.m = has_ep && nn > 1 ? nstep_finish<MODE>(rg, H, W, it.h, it.b, nn, E, far) : nn;
        it.cnt = max(0, min(Lc, it.m - it.t0));
        it.dA = dfirst - (W - 1);
        const int ok = __all(tid >= it.cnt || dmine - dfirst == tid);
        if ((tid & 63) == 0) flg[tid >> 6] = ok;
        __syncthreads();
        it.one = flg[0] & flg[1] & flg[2] & flg[3];
        __syncthreads();
    };
    f4 mk[PPT];
    float ac[PPT];
    // the staging loads of a joint item, nothing waited (a lane past the item's pairs
    // repeats the last pair's action load, as the n-step kernel does)
    auto issue = [&](const Item& it) {
        if (it.cnt == 0 || !it.one) return;
        const int nd = W + it.cnt, P = R * nd;
        const int hA = ring_wrap(it.h + it.t0, H);         // t0 < m < H
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int q = min(tid + k * 256, P - 1);
            const int t = (int)fdiv((uint32_t)q, div_r), n = it.n0 + q - t * R;
            ac[k] = actions[((size_t)ring_wrap(hA + t, H) * B + it.b) * N + n];
            const int d = it.dA + t;
            const bool in = tid + k * 256 < P && t < nd - 1 && d >= 0 && d < T;
            mk[k] = buf_load4(rs_ser, in ? ((uint32_t)d * (uint32_t)N + (uint32_t)n) * 16u : 0xFFFFFFF0u);
        }
    };
    Item c, n1 = {}, n2 = {};
    bool v1 = (int)blockIdx.x + G < items, v2 = (int)blockIdx.x + 2 * G < items;
    int i2 = (int)blockIdx.x + 2 * G;                      // the item n2 describes
    raw((int)blockIdx.x, c);
    if (v1) raw((int)blockIdx.x + G, n1);
    if (v2) raw(i2, n2);
    resolve(c);
    if (v1) resolve(n1);
    issue(c);
    while (true) {
        const int nE = min(Lc, L - c.t0);                  // the chunk's elements, cnt of them live
        auto slot = [&](int t) {                           // element t of the chunk -> its output slot
            return time_major ? (int64_t)(c.t0 + t) * S + c.j : (int64_t)c.j * L + c.t0 + t;
        };
        // elements [tb, te) of the chunk from the image, element t at a shift of t - tsh days
        auto emit = [&](int tb, int te, int tsh) {
            for (int q = tid; q < per / 4; q += 256) {
                int off[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = 4 * q + k;
                    off[k] = (int)__umul24(fdiv((uint32_t)e, div_wf), skip) + e;
                }
                for (int t = tb; t < te; ++t) {
                    f4 v = f4{0.0f, 0.0f, 0.0f, 0.0f};
                    if (t < c.cnt) {
                        const float* p = img + (t - tsh) * F;
                        v = f4{p[off[0]], p[off[1]], p[off[2]], p[off[3]]};
                    }
                    float* xo = x + (slot(t) * N + c.n0) * WF;
                    buf_store4<NT>(make_rsrc(xo, (uint32_t)per * 4u), (uint32_t)q * 16u, v);
                }
            }
            for (int q = tid; q < (te - tb) * R; q += 256) {           // a = actions[h0+t+W]: image day W + t
                const int tq = (int)fdiv((uint32_t)q, div_r), nl = q - tq * R, t = tb + tq;
                a_out[slot(t) * N + c.n0 + nl] = t < c.cnt ? img[((size_t)nl * D + W + t - tsh) * F + 4] : 0.0f;
            }
        };
        if (c.n0 == 0) {
            const int hr = ring_wrap(ring_wrap(c.h + W - 1, H) + min(c.t0, H), H);   // used where t0 < m only
            for (int t = tid; t < nE; t += 256)
                r_out[slot(t)] = t < c.cnt ? rewards[(size_t)ring_wrap(hr + t, H) * B + c.b] : 0.0f;
            if (c.t0 == 0 && tid == 0) length[c.j] = c.m;
        }
        if (c.one) {
            const int nd = W + c.cnt, P = c.cnt ? R * nd : 0;
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const int q = tid + k * 256;
                if (q < P) {
                    const int t = (int)fdiv((uint32_t)q, div_r), nl = q - t * R;
                    const int d = c.dA + t;
                    const bool in = t < nd - 1 && d >= 0 && d < T;
                    float* dst = img + ((size_t)nl * D + t) * F;
                    dst[0] = in ? mk[k].x : NAN;
                    dst[1] = in ? mk[k].y : NAN;
                    dst[2] = in ? mk[k].z : NAN;
                    dst[3] = in ? mk[k].w : NAN;
                    dst[4] = ac[k];
                }
            }
            __syncthreads();
            if (v1) issue(n1);                             // the next item's loads fly during the write-out
            emit(0, nE, 0);
        } else {
            if (v1) issue(n1);
            // days that skip: each live element staged on its own (W days and W + 1 action rows)
            for (int t = 0; t < c.cnt; ++t) {
                const int ht = ring_wrap(ring_wrap(c.h + c.t0, H) + t, H);
                const int d0 = days[(size_t)ring_wrap(ht + W - 1, H) * B + c.b] - (W - 1);
                for (int q = tid; q < R * (W + 1); q += 256) {
                    const int p = (int)fdiv((uint32_t)q, div_r), nl = q - p * R, n = c.n0 + nl;
                    const int d = d0 + p;
                    const bool in = p < W && d >= 0 && d < T;
                    f4 mv = f4{NAN, NAN, NAN, NAN};
                    if (in) mv = *reinterpret_cast<const f4*>(series + ((size_t)d * N + n) * 4);
                    float* dst = img + ((size_t)nl * D + p) * F;
                    dst[0] = mv.x;
                    dst[1] = mv.y;
                    dst[2] = mv.z;
                    dst[3] = mv.w;
                    dst[4] = actions[((size_t)ring_wrap(ht + p, H) * B + c.b) * N + n];
                }
                __syncthreads();
                emit(t, t + 1, t);
                __syncthreads();
            }
            emit(c.cnt, nE, 0);                            // zeros: no LDS read
        }
        // index chain ahead: the item after next completes, the one behind it loads env / h0
        Item n3 = {};
        const int i3 = i2 + G;
        const bool v3 = i3 < items;
        if (v3) raw(i3, n3);
        if (v2) resolve(n2);                               // its barriers also fence the image
        else __syncthreads();
        if (!v1) break;
        c = n1;
        n1 = n2; v1 = v2;
        n2 = n3; v2 = v3; i2 = i3;
    }
}

#define PMENV_SEQ_F5P_ARGS                                                                                           \
    const float *__restrict__ series, int T, int N, int W, const int32_t *__restrict__ days,                        \
        const float *__restrict__ actions, const float *__restrict__ rewards, int H, int B,                         \
        const int32_t *__restrict__ h0, const int32_t *__restrict__ env, int S, NstepRing rg, int Lc, int nc,       \
        int time_major, float *x, float *a_out, float *r_out, int32_t *length, int R, FastDiv div_r,                \
        FastDiv div_wf, FastDiv div_nc, FastDiv div_gy
// one id per ring row (rg.row_ep [H], or nullptr)
template <int PPT, int NT>
__global__ __launch_bounds__(256) void replay_seq_f5p_kernel(PMENV_SEQ_F5P_ARGS) {
    replay_seq_f5p_body<PPT, NT, kEpRow>(series, T, N, W, days, actions, rewards, H, B, h0, env, S, rg, Lc, nc,
                                         time_major, x, a_out, r_out, length, R, div_r, div_wf, div_nc, div_gy);
}
// one id per (ring row, env) (rg.row_ep [H, B], rg.stride_h = B)
template <int PPT, int NT>
__global__ __launch_bounds__(256) void replay_seq_f5p_env_kernel(PMENV_SEQ_F5P_ARGS) {
    replay_seq_f5p_body<PPT, NT, kEpEnv>(series, T, N, W, days, actions, rewards, H, B, h0, env, S, rg, Lc, nc,
                                         time_major, x, a_out, r_out, length, R, div_r, div_wf, div_nc, div_gy);
}
#undef PMENV_SEQ_F5P_ARGS

}  // namespace pmenv_dev
