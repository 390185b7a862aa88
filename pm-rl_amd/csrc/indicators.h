// indicators.h — the technical indicators of the feature pipeline (data/instrument.py:207-232:
// TA-Lib per ticker over f64 OHLCV; the definitions are include/pmenv.h's). bars is
// [T, N, C] f32, every element widened to f64 on load, all arithmetic f64 with contraction off
// (a product and a sum stay two roundings, as the numpy restatement computes them), every
// output rounded once to f32 into out[((t - L) * N + n) * ldo + col]. Three kinds of work:
//
//   pointwise   true range, directional movement, gain / loss, typical price, A/D and OBV
//               increments: device functions of rows t and t-1, never stored
//   windowed    ind_window_kernel<kind> (bbands, cci, stoch's two SMAs) and ind_fastk_kernel:
//               one thread per (row, column), one ascending chain per output
//   recurrences ind_step: every recurrence of a walk (ind_plan.h IndWalk: one op per kind)
//               advanced by one row; ind_scan_seq_kernel walks a column from row 0,
//               ind_scan_split_kernel walks row segments in three passes.
//
// ind_plan.h decides everything: the walks, the form, the segments, the workspace.
#pragma once

#include "common.h"
#include "ind_plan.h"

namespace pmenv_dev {

using namespace pmenv_host;

struct IndScanArgs {
    const float* bars;
    float* out;
    double* rec;                 // split records [n_seg, kIndSlots, N]
    int T, N, C, ldo, L;
    int ch[5];
    unsigned mask, need;
    int p[kIndKinds][3];
    int col[kIndKinds];          // col0 + the kind's first column
    int seg_len, n_seg;
    double apow[kIndSlots];      // a^seg_len of every slot's recurrence
};

struct IndWinArgs {
    const float* bars;
    float* out;
    double* fastk;               // stoch's fastk stream [T, N] f64 (rows >= fastk_period - 1)
    int T, N, C, ldo, L;
    int ch[5];
    int col;
    int p[3];
    double f[2];
};

struct IndRow {
    float h, l, c, v;
};

struct IndState {
    double s[kIndSlots];
    // the seeds' sums: rows at or before an op's lookback, so segment 0 and the sequential walk only
    double ema_sum, macd_fsum, macd_ssum, macd_gsum, atr_sum, rsi_gs, rsi_ls, adx_dsum;
};

// the larger of two values, NaN if either is NaN (numpy's maximum)
__device__ __forceinline__ double ind_max(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ double ind_min(double a, double b) { return (b < a || b != b) ? b : a; }

__device__ __forceinline__ bool ind_has(unsigned mask, int kind) { return (mask >> kind) & 1u; }

// dx of the three Wilder sums (deviation from TA-Lib: 0 where TA-Lib repeats its last value)
__device__ __forceinline__ double ind_dx(double sp, double sm, double str) {
#pragma clang fp contract(off)
    if (fabs(str) < 1e-8) return 0.0;
    const double dip = 100.0 * (sp / str), dim = 100.0 * (sm / str);
    const double sum = dim + dip;
    if (fabs(sum) < 1e-8) return 0.0;
    return 100.0 * (fabs(dim - dip) / sum);
}

// the three sums of dx / adx at row t >= 1: plain sums through t = p - 1, Wilder sums after
__device__ __forceinline__ void ind_dm_sums(double* s, int t, int p, double pdm, double mdm, double tr) {
#pragma clang fp contract(off)
    if (t <= p - 1) {
        s[0] += pdm;
        s[1] += mdm;
        s[2] += tr;
    } else {
        s[0] = s[0] - s[0] / p + pdm;
        s[1] = s[1] - s[1] / p + mdm;
        s[2] = s[2] - s[2] / p + tr;
    }
}

// Row t of every recurrence in the walk: x is row t, q row t - 1 (unused at t = 0). The
// seeding branches run at t <= the op's lookback only; behind it every slot is the linear
// s = a * s + b of its definition, which is what lets a segment start from zero or a carry.
template <bool EMIT>
__device__ __forceinline__ void ind_step(const IndScanArgs& a, IndState& st, int t, const IndRow& xr, const IndRow& qr,
                                         float* __restrict__ o) {
#pragma clang fp contract(off)
    const unsigned m = a.mask;
    const bool emit = EMIT && t >= a.L;
    const double h = (double)xr.h, l = (double)xr.l, c = (double)xr.c, v = (double)xr.v;
    const double qh = (double)qr.h, ql = (double)qr.l, qc = (double)qr.c;
    double* s = st.s;

    if (ind_has(m, PMENV_IND_EMA)) {
        const int p = a.p[PMENV_IND_EMA][0];
        const double k = 2.0 / (p + 1);
        if (t < p) {
            st.ema_sum += c;
            if (t == p - 1) s[kSlotEma] = st.ema_sum / p;
        } else {
            s[kSlotEma] = (c - s[kSlotEma]) * k + s[kSlotEma];
        }
        if (emit) o[a.col[PMENV_IND_EMA]] = (float)s[kSlotEma];
    }
    if (ind_has(m, PMENV_IND_MACD)) {
        const int pf = a.p[PMENV_IND_MACD][0], ps = a.p[PMENV_IND_MACD][1], pg = a.p[PMENV_IND_MACD][2];
        const double kf = 2.0 / (pf + 1), ks = 2.0 / (ps + 1), kg = 2.0 / (pg + 1);
        if (t <= ps - 1) {
            st.macd_ssum += c;
            if (t >= ps - pf) st.macd_fsum += c;
            if (t == ps - 1) {
                s[kSlotMacdFast] = st.macd_fsum / pf;
                s[kSlotMacdSlow] = st.macd_ssum / ps;
            }
        } else {
            s[kSlotMacdFast] = (c - s[kSlotMacdFast]) * kf + s[kSlotMacdFast];
            s[kSlotMacdSlow] = (c - s[kSlotMacdSlow]) * ks + s[kSlotMacdSlow];
        }
        if (t >= ps - 1) {
            const double mm = s[kSlotMacdFast] - s[kSlotMacdSlow];
            const int tg = ps - 1 + pg - 1;
            if (t <= tg) {
                st.macd_gsum += mm;
                if (t == tg) s[kSlotMacdSignal] = st.macd_gsum / pg;
            } else {
                s[kSlotMacdSignal] = (mm - s[kSlotMacdSignal]) * kg + s[kSlotMacdSignal];
            }
            if (emit) {
                float* oo = o + a.col[PMENV_IND_MACD];
                oo[0] = (float)mm;
                oo[1] = (float)s[kSlotMacdSignal];
                oo[2] = (float)(mm - s[kSlotMacdSignal]);
            }
        }
    }
    // pointwise values of rows t and t - 1
    double tr = 0.0, pdm = 0.0, mdm = 0.0;
    if ((m & ((1u << PMENV_IND_ATR) | (1u << PMENV_IND_DX) | (1u << PMENV_IND_ADX))) && t >= 1) {
        tr = ind_max(ind_max(h - l, fabs(h - qc)), fabs(l - qc));
        const double up = h - qh, dn = ql - l;
        if (dn > 0.0 && up < dn) mdm = dn;
        else if (up > 0.0 && up > dn) pdm = up;
    }
    if (ind_has(m, PMENV_IND_ATR)) {
        const int p = a.p[PMENV_IND_ATR][0];
        if (t >= 1) {
            if (t <= p) {
                st.atr_sum += tr;
                if (t == p) s[kSlotAtr] = st.atr_sum / p;
            } else {
                s[kSlotAtr] = (s[kSlotAtr] * (p - 1) + tr) / p;
            }
        }
        if (emit) o[a.col[PMENV_IND_ATR]] = (float)s[kSlotAtr];
    }
    if (ind_has(m, PMENV_IND_RSI)) {
        const int p = a.p[PMENV_IND_RSI][0];
        if (t >= 1) {
            const double gain = ind_max(c - qc, 0.0), loss = ind_max(qc - c, 0.0);
            if (t <= p) {
                st.rsi_gs += gain;
                st.rsi_ls += loss;
                if (t == p) {
                    s[kSlotRsiGain] = st.rsi_gs / p;
                    s[kSlotRsiLoss] = st.rsi_ls / p;
                }
            } else {
                s[kSlotRsiGain] = (s[kSlotRsiGain] * (p - 1) + gain) / p;
                s[kSlotRsiLoss] = (s[kSlotRsiLoss] * (p - 1) + loss) / p;
            }
        }
        if (emit) {
            const double den = s[kSlotRsiGain] + s[kSlotRsiLoss];
            o[a.col[PMENV_IND_RSI]] = (float)(fabs(den) < 1e-8 ? 0.0 : 100.0 * (s[kSlotRsiGain] / den));
        }
    }
    if (ind_has(m, PMENV_IND_DX)) {
        const int p = a.p[PMENV_IND_DX][0];
        if (t >= 1) ind_dm_sums(s + kSlotDxPlus, t, p, pdm, mdm, tr);
        if (emit) o[a.col[PMENV_IND_DX]] = (float)ind_dx(s[kSlotDxPlus], s[kSlotDxMinus], s[kSlotDxTr]);
    }
    if (ind_has(m, PMENV_IND_ADX)) {
        const int p = a.p[PMENV_IND_ADX][0];
        if (t >= 1) ind_dm_sums(s + kSlotAdxPlus, t, p, pdm, mdm, tr);
        if (t >= p) {
            const double dx = ind_dx(s[kSlotAdxPlus], s[kSlotAdxMinus], s[kSlotAdxTr]);
            if (t <= 2 * p - 1) {
                st.adx_dsum += dx;
                if (t == 2 * p - 1) s[kSlotAdx] = st.adx_dsum / p;
            } else {
                s[kSlotAdx] = (s[kSlotAdx] * (p - 1) + dx) / p;
            }
        }
        if (emit) o[a.col[PMENV_IND_ADX]] = (float)s[kSlotAdx];
    }
    if (ind_has(m, PMENV_IND_OBV)) {
        if (t == 0) s[kSlotObv] = v;
        else s[kSlotObv] += c > qc ? v : (c < qc ? -v : 0.0);
        if (emit) o[a.col[PMENV_IND_OBV]] = (float)s[kSlotObv];
    }
    if (ind_has(m, PMENV_IND_ADOSC)) {
        const double kf = 2.0 / (a.p[PMENV_IND_ADOSC][0] + 1), ks = 2.0 / (a.p[PMENV_IND_ADOSC][1] + 1);
        const double hl = h - l;
        const double inc = hl > 0.0 ? ((c - l) - (h - c)) / hl * v : 0.0;
        if (t == 0) {
            s[kSlotAd] = inc;
            s[kSlotAdFast] = s[kSlotAd];
            s[kSlotAdSlow] = s[kSlotAd];
        } else {
            s[kSlotAd] += inc;
            s[kSlotAdFast] = kf * s[kSlotAd] + (1.0 - kf) * s[kSlotAdFast];
            s[kSlotAdSlow] = ks * s[kSlotAd] + (1.0 - ks) * s[kSlotAdSlow];
        }
        if (emit) o[a.col[PMENV_IND_ADOSC]] = (float)(s[kSlotAdFast] - s[kSlotAdSlow]);
    }
}

// Rows [t0, t1) of column n, four at a time: the next four rows are loaded before the
// current four are stepped, so a step does not wait for its own row. Row indices are
// clamped to T - 1 (what a clamped load returns is never stepped).
template <bool EMIT>
__device__ __forceinline__ void ind_walk(const IndScanArgs& a, IndState& st, int64_t n, int t0, int t1) {
    const int64_t last = (int64_t)a.T - 1;
    auto ld = [&](int64_t t) {
        const float* p = a.bars + ((size_t)(t > last ? last : t) * (size_t)a.N + (size_t)n) * (size_t)a.C;
        IndRow r;
        r.h = (a.need & kIndH) ? p[a.ch[1]] : 0.0f;
        r.l = (a.need & kIndL) ? p[a.ch[2]] : 0.0f;
        r.c = (a.need & kIndC) ? p[a.ch[3]] : 0.0f;
        r.v = (a.need & kIndV) ? p[a.ch[4]] : 0.0f;
        return r;
    };
    IndRow prev = ld(t0 > 0 ? t0 - 1 : 0);
    IndRow nxt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) nxt[i] = ld((int64_t)t0 + i);
    for (int64_t t = t0; t < t1; t += 4) {
        IndRow cur[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) nxt[i] = ld(t + 4 + i);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (t + i < t1) {
                const int64_t r = t + i - a.L;       // the output row; o is used at r >= 0 only
                float* o = a.out + ((size_t)(r > 0 ? r : 0) * (size_t)a.N + (size_t)n) * (size_t)a.ldo;
                ind_step<EMIT>(a, st, (int)(t + i), cur[i], prev, o);
                prev = cur[i];
            }
        }
    }
}

__device__ __forceinline__ void ind_state_zero(IndState& st) {
#pragma unroll
    for (int i = 0; i < kIndSlots; ++i) st.s[i] = 0.0;
    st.ema_sum = st.macd_fsum = st.macd_ssum = st.macd_gsum = 0.0;
    st.atr_sum = st.rsi_gs = st.rsi_ls = st.adx_dsum = 0.0;
}

// The many-columns form: one lane per column, rows 0 .. T-1, coalesced across the lanes.
static __global__ __launch_bounds__(64) void ind_scan_seq_kernel(IndScanArgs a) {
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (n >= a.N) return;
    IndState st;
    ind_state_zero(st);
    ind_walk<true>(a, st, n, 0, a.T);
}

// The few-columns form. Segment 0 is rows [0, L + seg_len), segment j >= 1 rows
// [L + j * seg_len, L + (j + 1) * seg_len) cut at T: behind the lookback, where every slot is
// linear. rec[j][slot][n] is segment 0's state at its end (absolute) and, for j >= 1, the
// segment's end state from a zero carry (local); the carry into segment j is composed in
// segment order, c = a^seg_len * c + local.
//   PASS 1  grid.y = n_seg      segment 0: the sequential walk with its outputs, all slots
//                               recorded; j >= 1: level-1 slots from zero
//   PASS 2  grid.y = n_seg - 1  j >= 1: level-1 slots from their carry, level-2 slots from zero
//                               (only when the walk has a level-2 kind)
//   PASS 3  grid.y = n_seg - 1  j >= 1: every slot from its carry, outputs written
template <int PASS>
static __global__ __launch_bounds__(64) void ind_scan_split_kernel(IndScanArgs a) {
#pragma clang fp contract(off)
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (n >= a.N) return;
    const int j = (int)blockIdx.y + (PASS == 1 ? 0 : 1);
    const int64_t lo = (int64_t)a.L + (int64_t)j * a.seg_len, hi = lo + a.seg_len;
    const int t0 = j == 0 ? 0 : (int)lo, t1 = (int)(hi < a.T ? hi : a.T);
    auto rec = [&](int seg, int slot) -> double& {
        return a.rec[((size_t)seg * kIndSlots + (size_t)slot) * (size_t)a.N + (size_t)n];
    };
    IndState st;
    ind_state_zero(st);
    if (PASS == 1) {
        if (j == 0) ind_walk<true>(a, st, n, t0, t1);
        else ind_walk<false>(a, st, n, t0, t1);
#pragma unroll
        for (int i = 0; i < kIndSlots; ++i)
            if (ind_has(a.mask, ind_slot_kind(i)) && (j == 0 || i < kIndLevel1)) rec(j, i) = st.s[i];
        return;
    }
#pragma unroll
    for (int i = 0; i < (PASS == 2 ? (int)kIndLevel1 : (int)kIndSlots); ++i) {
        if (!ind_has(a.mask, ind_slot_kind(i))) continue;
        double c = rec(0, i);
        for (int q = 1; q < j; ++q) c = a.apow[i] * c + rec(q, i);
        st.s[i] = c;
    }
    if (PASS == 2) {
        ind_walk<false>(a, st, n, t0, t1);
#pragma unroll
        for (int i = kIndLevel1; i < kIndSlots; ++i)
            if (ind_has(a.mask, ind_slot_kind(i))) rec(j, i) = st.s[i];
    } else {
        ind_walk<true>(a, st, n, t0, t1);
    }
}

// ---------------------------------------------------------------- the windowed ops
// stoch's fastk at every row t >= fastk_period - 1, f64: (c - LL) / ((HH - LL) / 100) over
// the trailing highs and lows, 0 where HH == LL. One thread per (row, column).
static __global__ __launch_bounds__(kIndWindowBlock) void ind_fastk_kernel(IndWinArgs a) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * kIndWindowBlock + threadIdx.x;
    if (idx >= (int64_t)a.T * a.N) return;
    const int64_t t = idx / a.N, n = idx - t * a.N;
    const int p = a.p[0];
    if (t < p - 1) return;
    auto at = [&](int64_t tt, int ch) {
        return (double)a.bars[((size_t)tt * (size_t)a.N + (size_t)n) * (size_t)a.C + (size_t)ch];
    };
    double hh = at(t - p + 1, a.ch[1]), ll = at(t - p + 1, a.ch[2]);
    for (int64_t i = t - p + 2; i <= t; ++i) {
        hh = ind_max(hh, at(i, a.ch[1]));
        ll = ind_min(ll, at(i, a.ch[2]));
    }
    const double c = at(t, a.ch[3]);
    a.fastk[idx] = hh == ll ? 0.0 : (c - ll) / ((hh - ll) / 100.0);
}

// One thread per (output row, column): the sums ascend over the trailing p rows.
template <int KIND>
static __global__ __launch_bounds__(kIndWindowBlock) void ind_window_kernel(IndWinArgs a) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * kIndWindowBlock + threadIdx.x;
    if (idx >= ((int64_t)a.T - a.L) * a.N) return;
    const int64_t r = idx / a.N, n = idx - r * a.N, t = a.L + r;
    auto at = [&](int64_t tt, int ch) {
        return (double)a.bars[((size_t)tt * (size_t)a.N + (size_t)n) * (size_t)a.C + (size_t)ch];
    };
    float* o = a.out + (size_t)idx * (size_t)a.ldo + a.col;
    if (KIND == PMENV_IND_BBANDS) {
        const int p = a.p[0];
        double sum = 0.0, sq = 0.0;
        for (int64_t i = t - p + 1; i <= t; ++i) {
            const double x = at(i, a.ch[3]);
            sum += x;
            sq += x * x;
        }
        const double mean = sum / p;
        const double var = sq / p - mean * mean;
        const double sd = var > 0.0 ? sqrt(var) : 0.0;
        o[0] = (float)(mean + a.f[0] * sd);
        o[1] = (float)mean;
        o[2] = (float)(mean - a.f[1] * sd);
    } else if (KIND == PMENV_IND_CCI) {
        const int p = a.p[0];
        auto tp = [&](int64_t i) { return (at(i, a.ch[1]) + at(i, a.ch[2]) + at(i, a.ch[3])) / 3.0; };
        double sum = 0.0;
        for (int64_t i = t - p + 1; i <= t; ++i) sum += tp(i);
        const double mean = sum / p;
        double md = 0.0;
        for (int64_t i = t - p + 1; i <= t; ++i) md += fabs(tp(i) - mean);
        md = md / p;
        const double x = tp(t);
        o[0] = (float)((x == mean || md == 0.0) ? 0.0 : (x - mean) / (0.015 * md));
    } else {                                        // PMENV_IND_STOCH: slowk, slowd of the fastk stream
        const int sk = a.p[1], sd = a.p[2];
        auto slowk = [&](int64_t tt) {
            double sum = 0.0;
            for (int64_t i = tt - sk + 1; i <= tt; ++i) sum += a.fastk[(size_t)i * (size_t)a.N + (size_t)n];
            return sum / sk;
        };
        double sum = 0.0;
        for (int64_t i = t - sd + 1; i <= t; ++i) sum += slowk(i);
        o[0] = (float)slowk(t);
        o[1] = (float)(sum / sd);
    }
}

}  // namespace pmenv_dev
