// adf.h — the search for the orders of differencing on the device (data/ffd.py:59-78, the
// reference's FixedFracDiff.fit: a bisection per column whose every probe is one conv1d and
// one statsmodels adfuller call on the host): the per-column tap table of ffd.py:38-47, a
// batched augmented Dickey-Fuller statistic and the bisection's state update. adf_plan.h
// holds the lag rule, the p-value, the geometry and the workspace; include/pmenv.h the
// definitions these kernels implement.
#pragma once

#include "adf_plan.h"
#include "common.h"

namespace pmenv_dev {

using pmenv_host::adf_maxlag;
using pmenv_host::adf_pvalue;
using pmenv_host::kAdfChunk;
using pmenv_host::kAdfMinRows;
using pmenv_host::kAdfTableBlock;
using pmenv_host::kAdfTile;

// ---------------------------------------------------------------- the tap table
// pmenv_ffd_weights per column, one lane each: the same f32 factors ((0 - f32(d + 1)) / k + 1,
// a correctly rounded f32 divide), the same f64 running product rounded once per tap, the
// same width rule over all T - 1 taps. Lanes are columns, so a tap row is one coalesced
// store. Rows >= width are zeroed; a d that pmenv_ffd_weights refuses (negative, not finite)
// gives width 0.
static __global__ __launch_bounds__(kAdfTableBlock) void ffd_table_kernel(const double* __restrict__ d, double thres,
                                                                        int T, int C, int cap,
                                                                        float* __restrict__ taps,
                                                                        int32_t* __restrict__ width) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * kAdfTableBlock + threadIdx.x;
    if (c >= C) return;
    const double dv = d[c];
    const float th = (float)thres;
    int w = 0;
    if (dv > 0.0 && isfinite(dv)) {
        const float neg = 0.0f - (float)(dv + 1.0);
        double prod = 1.0;
        if (cap > 0) taps[c] = 1.0f;
        for (int k = 1; k < T; ++k) {
            const float q = neg / (float)k;
            prod *= (double)(q + 1.0f);
            const float tap = (float)prod;
            if (fabsf(tap) > th) w = k;
            if (k < cap) taps[(size_t)k * (size_t)C + (size_t)c] = tap;
            if (prod == 0.0) break;
        }
    }
    for (int k = w; k < cap; ++k) taps[(size_t)k * (size_t)C + (size_t)c] = 0.0f;
    width[c] = w;
}

// ---------------------------------------------------------------- the ADF statistic: the long sums
// Column c is x[i] = y[(first[c] + i) * ld + c], i < n = R - first[c], K its lag bound
// (adf_maxlag). With z[i] = x[i] - m and e[i] = x[i+1] - x[i] - (x[n-1] - x[0]) / (n - 1) — the
// level and the differences, each shifted by a constant near its mean so that the centring
// of the Gram matrix below cancels nothing: m is the mean of 64 rows spread evenly over the
// column (x[0] alone sits a couple of deviations off the mean of a drifting walk, and the
// centred entries would lose that factor squared) — the fit on rows t = K .. n-2 needs
//     A_r = sum e[t] e[t-r], L_r = sum z[t] e[t-r]  (r = 0 .. K),  sum z^2, sum z, sum e[t]:
// every other product of two lagged differences is one of the A_r plus a few terms at the
// two ends (adf_solve_kernel). A workgroup takes a tile of kAdfTile columns, one wave each:
// all its threads stage kAdfChunk rows of the tile (a row of the tile is one contiguous
// segment of y) as f64 e into a ring of two chunks and z into a chunk buffer in LDS, then
// wave w walks its column's rows of the chunk with lane l holding sums l, l + 64, l + 128 of
// the 2K + 5. Each sum is one chain acc = fma(a, b, acc) over ascending t, carried across the
// chunks: its bits depend on no tile, no chunk boundary, no other column and not on first[c].
// work[c * rec + s] takes sum s, work[c * rec + 2K + 5] is 1 where a row of the column is not
// finite, work[c * rec + 2K + 6] is m. A column below kAdfMinRows rows writes nothing.
static __global__ __launch_bounds__(64 * kAdfTile) void adf_sums_kernel(const float* __restrict__ y,
                                                                       const int32_t* __restrict__ first, int R,
                                                                       int C, int ld, int maxlag, int rec,
                                                                       double* __restrict__ work) {
    __shared__ double ring[kAdfTile][2 * kAdfChunk];
    __shared__ double zbuf[kAdfTile][kAdfChunk];
    __shared__ int bad[kAdfTile];
    __shared__ double shift[kAdfTile];
    constexpr int kRing = 2 * kAdfChunk - 1, kZ = kAdfChunk - 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto first_of = [&](int64_t c) {
        const int f = first ? first[c] : 0;
        return f < 0 ? 0 : (f > R ? R : f);
    };
    // the first row any column of the tile uses
    const int64_t c0 = (int64_t)blockIdx.x * kAdfTile;
    int a_lo = R;
    for (int i = 0; i < kAdfTile; ++i)
        if (c0 + i < C) a_lo = min(a_lo, first_of(c0 + i));
    // the loader's column: thread -> (row tid / 8 of a 64-row step, column tid % 8)
    const int lc = tid & (kAdfTile - 1), lr = tid / kAdfTile;
    const int64_t cl = c0 + lc;
    const bool l_ok = cl < C;
    const int f_l = l_ok ? first_of(cl) : R;
    const int n_l = R - f_l;
    double md_l = 0.0;
    if (n_l >= 2)
        md_l = ((double)y[(size_t)(R - 1) * (size_t)ld + (size_t)cl] - (double)y[(size_t)f_l * (size_t)ld + (size_t)cl]) /
               (double)(n_l - 1);
    // the wave's column and its lanes' sums
    const int64_t cw = c0 + wave;
    const int f_w = cw < C ? first_of(cw) : R;
    const int n_w = R - f_w;
    const bool live = n_w >= kAdfMinRows;
    const int K = live ? (int)adf_maxlag(n_w, maxlag) : 0;
    const int nsum = 2 * K + 5;
    int r[3], mode[3];          // mode 0: b = e[t - r]; 1: b = z[t]; 2: b = 1; 3: no sum
    bool az[3];                 // a = z[t] (else e[t])
    double acc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int s = lane + 64 * j;
        acc[j] = 0.0;
        r[j] = 0;
        az[j] = false;
        mode[j] = 3;
        if (!live) continue;
        if (s <= K) {
            mode[j] = 0; r[j] = s;
        } else if (s <= 2 * K + 1) {
            mode[j] = 0; r[j] = s - K - 1; az[j] = true;
        } else if (s == 2 * K + 2) {
            mode[j] = 1; az[j] = true;
        } else if (s == 2 * K + 3) {
            mode[j] = 2; az[j] = true;
        } else if (s == 2 * K + 4) {
            mode[j] = 2;
        }
    }
    // the level's shift: lane k reads row k (n - 1) / 63 of the wave's column, one butterfly sum
    double m = 0.0;
    if (live) {
        m = (double)y[(size_t)(f_w + (int)(((int64_t)lane * (n_w - 1)) / 63)) * (size_t)ld + (size_t)cw];
        for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
        m *= 1.0 / 64.0;
    }
    if (lane == 0) shift[wave] = m;
    if (tid < kAdfTile) bad[tid] = 0;
    __syncthreads();
    const double x0_l = shift[lc];

    for (int a0 = a_lo; a0 < R - 1; a0 += kAdfChunk) {
        // stage rows a0 .. a0 + kAdfChunk - 1 (up to R - 2, the last row with a difference)
#pragma unroll
        for (int s = 0; s < kAdfChunk * kAdfTile / (64 * kAdfTile); ++s) {
            const int a = a0 + lr + 64 * s;
            if (l_ok && a >= f_l && a <= R - 2) {
                const float xa = y[(size_t)a * (size_t)ld + (size_t)cl];
                const float xb = y[(size_t)(a + 1) * (size_t)ld + (size_t)cl];
                if (!isfinite(xa) || (a == R - 2 && !isfinite(xb))) bad[lc] = 1;
                ring[lc][a & kRing] = (double)xb - (double)xa - md_l;
                zbuf[lc][a & kZ] = (double)xa - x0_l;
            }
        }
        __syncthreads();
        if (live) {
            const int lo = max(a0, f_w + K), hi = min(a0 + kAdfChunk - 1, R - 2);
            for (int a = lo; a <= hi; ++a) {
                const double et = ring[wave][a & kRing], zt = zbuf[wave][a & kZ];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if (mode[j] == 3) continue;
                    const double av = az[j] ? zt : et;
                    const double bv = mode[j] == 0 ? ring[wave][(a - r[j]) & kRing] : (mode[j] == 1 ? zt : 1.0);
                    acc[j] = fma(av, bv, acc[j]);
                }
            }
        }
        __syncthreads();                 // the next step overwrites the older half of the ring
    }
    if (!live) return;
    double* out = work + (size_t)cw * (size_t)rec;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int s = lane + 64 * j;
        if (s < nsum) out[s] = acc[j];
    }
    if (lane == 0) {
        out[nsum] = bad[wave] ? 1.0 : 0.0;
        out[nsum + 1] = m;
    }
}

// ---------------------------------------------------------------- the ADF statistic: the fits
// packed lower triangle
static __device__ __forceinline__ int adf_tri(int i, int l) { return i * (i + 1) / 2 + l; }

// In-place right-looking Cholesky of the packed mm x mm matrix G in LDS by one wave: pivot j
// scales its column, then every entry (i, l) below loses L_ij * L_lj — entry (i, l) sees its
// subtractions in ascending j, whatever lane holds it. false (for all lanes) at a pivot that
// is not a positive finite number.
static __device__ bool adf_cholesky(double* G, int mm, int lane) {
    for (int j = 0; j < mm; ++j) {
        __syncthreads();
        const double p = G[adf_tri(j, j)];
        if (!(p > 0.0) || !isfinite(p)) return false;
        const double sq = sqrt(p);
        for (int i = j + 1 + lane; i < mm; i += 64) G[adf_tri(i, j)] = G[adf_tri(i, j)] / sq;
        __syncthreads();
        if (lane == 0) G[adf_tri(j, j)] = sq;
        for (int i = j + 1; i < mm; ++i) {
            const double lij = G[adf_tri(i, j)];
            for (int l = j + 1 + lane; l <= i; l += 64) G[adf_tri(i, l)] = fma(-lij, G[adf_tri(l, j)], G[adf_tri(i, l)]);
        }
    }
    __syncthreads();
    return true;
}

// One wave per column. From the sums of adf_sums_kernel and the K + 2 rows at either end of
// the column it forms Q[a][b] = sum_{t=K}^{n-2} e[t-a] e[t-b] (a <= b <= K: diagonal r = b - a
// starts at A_r and moves one row up per step, adding the product at the head and dropping
// the one at the tail) and the sums of e[t-a] likewise. A fit with L lags on rows s .. n-2
// (s <= K) is then the centred Gram matrix
//     G[j][l] = P[j][l] + (rows s .. K-1 of v_j v_l) - S_j S_l / nobs,   nobs = n - 1 - s,
// of its columns v in the given order, factored by adf_cholesky.
//   autolag: columns [level, lag 1 .. lag K | response] on rows K ..: the models are nested in
//     that order, so ssr_k = sum_{j > k} L_yj^2 for every k from the one factor; AIC_k =
//     nobs ln(ssr_k / nobs) + 2 (k + 2), the smallest k of the smallest AIC is usedlag.
//   final: columns [lag 1 .. lag u, level | response] on rows u ..: with the level last,
//     beta = L_y,level / L_level,level and [(X'X)^-1]_level = 1 / L_level,level^2, so
//     stat = L_y,level / sqrt(ssr / (nobs - u - 2)), ssr = L_yy^2.
// LDS (dynamic, adf_solve_doubles(kcap) doubles): Q, G and seven vectors of kcap + 2.
static __global__ __launch_bounds__(64) void adf_solve_kernel(const float* __restrict__ y,
                                                             const int32_t* __restrict__ first, int R, int C, int ld,
                                                             int maxlag, int autolag, int kcap, int rec,
                                                             const double* __restrict__ work,
                                                             double* __restrict__ stat, double* __restrict__ pvalue,
                                                             int32_t* __restrict__ usedlag,
                                                             int32_t* __restrict__ nobs_out,
                                                             int32_t* __restrict__ status) {
    extern __shared__ double adf_lds[];
    const int lane = threadIdx.x;
    const size_t c = blockIdx.x;
    int f = first ? first[c] : 0;
    f = f < 0 ? 0 : (f > R ? R : f);
    const int n = R - f;
    auto finish = [&](int st, double s, int u, int nobs) {
        if (lane == 0) {
            stat[c] = s;
            pvalue[c] = st == PMENV_ADF_OK ? adf_pvalue(s) : (double)NAN;
            usedlag[c] = u;
            nobs_out[c] = nobs;
            status[c] = st;
        }
    };
    if (n < kAdfMinRows) return finish(PMENV_ADF_TOO_SHORT, (double)NAN, 0, 0);
    const int K = (int)adf_maxlag(n, maxlag);
    const double* sums = work + c * (size_t)rec;
    if (sums[2 * K + 5] != 0.0) return finish(PMENV_ADF_DEGENERATE, (double)NAN, 0, 0);

    const int vlen = kcap + 2;
    double* Q = adf_lds;
    double* G = Q + (kcap + 1) * (kcap + 2) / 2;
    double* eh = G + (kcap + 2) * (kcap + 3) / 2;    // eh[i] = e[i], i <= K
    double* et = eh + vlen;                          // et[j] = e[n-2-j], j <= K
    double* zh = et + vlen;                          // zh[i] = z[i], i <= K
    double* Lz = zh + vlen;                          // Lz[a] = sum z[t] e[t-a]
    double* Sd = Lz + vlen;                          // Sd[a] = sum e[t-a]
    double* Sf = Sd + vlen;                          // the sums of the fit in hand; then ssr_k
    double* ly = Sf + vlen;                          // the response's row of the factor
    auto X = [&](int i) { return (double)y[(size_t)(f + i) * (size_t)ld + c]; };
    const double x0 = sums[2 * K + 6], md = (X(n - 1) - X(0)) / (double)(n - 1);   // the shifts of adf_sums_kernel
    for (int i = lane; i <= K; i += 64) {            // K + 1 <= n / 2 - 1: both ends stay inside the column
        const double xa = X(i);
        eh[i] = X(i + 1) - xa - md;
        zh[i] = xa - x0;
        et[i] = X(n - 1 - i) - X(n - 2 - i) - md;
        Lz[i] = sums[K + 1 + i];
    }
    __syncthreads();
    const double Zz = sums[2 * K + 2], Sz = sums[2 * K + 3];
    if (lane == 0) {
        double s = sums[2 * K + 4];
        Sd[0] = s;
        for (int a = 1; a <= K; ++a) {               // rows K-a .. n-2-a: one more at the head, one less at the tail
            s = (s + eh[K - a]) - et[a - 1];
            Sd[a] = s;
        }
    }
    for (int r = lane; r <= K; r += 64) {
        double v = sums[r];
        Q[adf_tri(r, 0)] = v;
        for (int a = 1; a + r <= K; ++a) {
            v = fma(eh[K - a], eh[K - a - r], v);
            v = fma(-et[a - 1], et[a - 1 + r], v);
            Q[adf_tri(a + r, a)] = v;
        }
    }
    __syncthreads();

    // column j of a fit with L lags and the level at position lp: -1 the level, else its lag (0: the response)
    auto code = [](int j, int L, int lp) { return j == lp ? -1 : (j == L + 1 ? 0 : (j < lp ? j + 1 : j)); };
    auto build = [&](int L, int lp) {
        const int mm = L + 2;
        const double nobs = (double)(n - 1 - L);
        for (int j = lane; j < mm; j += 64) {
            const int a = code(j, L, lp);
            double s = a < 0 ? Sz : Sd[a];
            for (int i = L; i < K; ++i) s += a < 0 ? zh[i] : eh[i - a];
            Sf[j] = s;
        }
        __syncthreads();
        for (int j = 0; j < mm; ++j) {
            const int a = code(j, L, lp);
            for (int l = lane; l <= j; l += 64) {
                const int b = code(l, L, lp);
                double v = a < 0 ? (b < 0 ? Zz : Lz[b]) : (b < 0 ? Lz[a] : Q[adf_tri(a > b ? a : b, a > b ? b : a)]);
                for (int i = L; i < K; ++i) v = fma(a < 0 ? zh[i] : eh[i - a], b < 0 ? zh[i] : eh[i - b], v);
                G[adf_tri(j, l)] = v - Sf[j] * Sf[l] / nobs;
            }
        }
    };

    int u = K;
    if (autolag && K > 0) {
        build(K, 0);
        if (!adf_cholesky(G, K + 2, lane)) return finish(PMENV_ADF_DEGENERATE, (double)NAN, 0, 0);
        for (int j = lane; j <= K + 1; j += 64) ly[j] = G[adf_tri(K + 1, j)];
        __syncthreads();
        if (lane == 0) {
            double s = ly[K + 1] * ly[K + 1];
            Sf[K] = s;
            for (int k = K - 1; k >= 0; --k) {
                s = fma(ly[k + 1], ly[k + 1], s);
                Sf[k] = s;
            }
        }
        __syncthreads();
        const double nobs = (double)(n - 1 - K);
        double best = INFINITY;
        bool okay = true;
        for (int k = 0; k <= K; ++k) {               // every lane: the same values in the same order
            const double ssr = Sf[k];
            if (!(ssr > 0.0) || !isfinite(ssr)) okay = false;
            const double aic = nobs * log(ssr / nobs) + 2.0 * (double)(k + 2);
            if (aic < best) {
                best = aic;
                u = k;
            }
        }
        __syncthreads();
        if (!okay) return finish(PMENV_ADF_DEGENERATE, (double)NAN, 0, 0);
    }
    build(u, u);
    if (!adf_cholesky(G, u + 2, lane)) return finish(PMENV_ADF_DEGENERATE, (double)NAN, 0, 0);
    const double lyy = G[adf_tri(u + 1, u + 1)], lyx = G[adf_tri(u + 1, u)];
    const int nobs = n - 1 - u;
    const double ssr = lyy * lyy;
    if (!(ssr > 0.0) || !isfinite(ssr)) return finish(PMENV_ADF_DEGENERATE, (double)NAN, 0, 0);
    const double s = lyx / sqrt(ssr / (double)(nobs - u - 2));
    if (!isfinite(s)) return finish(PMENV_ADF_DEGENERATE, (double)NAN, 0, 0);
    finish(PMENV_ADF_OK, s, u, nobs);
}

// ---------------------------------------------------------------- the bisection's state
// ffd.py:59-78 for one column per thread. p NULL: the first round (nothing probed yet).
// Otherwise the column's probe at d_opt gave p[c] / stat[c] / adf_status[c]: TOO_SHORT counts
// as p = 1; p > 0.05 moves low up, p < 0.049 moves high down, anything else — the band, a NaN
// — ends the column at d_opt. A column still active takes d_mid = (low + high) / 2: below
// thres it ends at 0, within thres of d_opt it ends there, otherwise d_opt = d_mid is the next
// probe. d[c] = d_opt in every case, so the next tap table is valid for every column.
static __global__ __launch_bounds__(256) void adf_search_update_kernel(
    const double* __restrict__ p, const double* __restrict__ stat, const int32_t* __restrict__ adf_status, double thres,
    int C, double* __restrict__ low, double* __restrict__ high, double* __restrict__ d_opt, int32_t* __restrict__ active,
    int32_t* __restrict__ evals, int32_t* __restrict__ status, double* __restrict__ last, double* __restrict__ d) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double lo = low[c], hi = high[c], dopt = d_opt[c];
    int act = active[c];
    if (act) {
        if (p) {
            const int st = adf_status[c];
            const double pv = p[c], pe = st == PMENV_ADF_TOO_SHORT ? 1.0 : pv;
            status[c] = st;
            if (last) {
                last[c] = pv;
                last[(size_t)C + c] = stat[c];
            }
            if (pe > pmenv_host::kAdfPHigh) lo = dopt;
            else if (pe < pmenv_host::kAdfPLow) hi = dopt;
            else act = 0;
        }
        if (act) {
            const double mid = (lo + hi) / 2.0;
            if (mid < thres) {
                dopt = 0.0;
                act = 0;
            } else if (fabs(dopt - mid) < thres) {
                act = 0;
            } else {
                dopt = mid;
                evals[c] += 1;
            }
        }
        low[c] = lo;
        high[c] = hi;
        d_opt[c] = dopt;
        active[c] = act;
    }
    d[c] = dopt;
}

}  // namespace pmenv_dev
