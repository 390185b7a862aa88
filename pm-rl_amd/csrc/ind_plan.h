// ind_plan.h — the technical-indicator stage of the feature pipeline on the host: the
// parameters, output count and lookback of every op (data/instrument.py:207-232 runs TA-Lib
// per ticker; the definitions are those of include/pmenv.h), and every decision of
// pmenv_ind_apply — which ops share a walk, which form the recurrences take, the split
// form's segments, the workspace layout, the kernels' names. pmenv_ind_layout,
// pmenv_ind_workspace, pmenv_ind_apply and pmenv_ind_path all read the one IndPlan built
// here. Host only and pure: no HIP header, no HIP call (it compiles with a plain host
// compiler), all products in int64.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/pmenv.h"

namespace pmenv_host {

constexpr int kIndKinds = 11;          // PMENV_IND_EMA .. PMENV_IND_ADOSC
constexpr int kIndMaxOps = 32;         // ops per call
constexpr int kIndMaxPeriod = 256;     // every period argument: 2 <= p <= 256
constexpr int kIndWindowBlock = 256;   // threads of ind_window_kernel / ind_fastk_kernel: one (row, column) each

// channel bits of chan[5] = {open, high, low, close, volume}
constexpr unsigned kIndO = 1, kIndH = 2, kIndL = 4, kIndC = 8, kIndV = 16;

// ---- the recurrences' state slots: one f64 per (column, slot). Level 1 reads the bars
// alone; level 2 reads level-1 values (the MACD signal, ADX, the two EMAs of the A/D line).
enum IndSlot {
    kSlotEma = 0,
    kSlotMacdFast, kSlotMacdSlow,
    kSlotAtr,
    kSlotRsiGain, kSlotRsiLoss,
    kSlotDxPlus, kSlotDxMinus, kSlotDxTr,
    kSlotAdxPlus, kSlotAdxMinus, kSlotAdxTr,
    kSlotObv,
    kSlotAd,
    kIndLevel1,                          // 14 level-1 slots
    kSlotMacdSignal = kIndLevel1,
    kSlotAdx,
    kSlotAdFast, kSlotAdSlow,
    kIndSlots                            // 18
};

// the kind that owns a slot
constexpr int ind_slot_kind(int slot) {
    return slot == kSlotEma ? PMENV_IND_EMA
         : slot == kSlotMacdFast || slot == kSlotMacdSlow || slot == kSlotMacdSignal ? PMENV_IND_MACD
         : slot == kSlotAtr ? PMENV_IND_ATR
         : slot == kSlotRsiGain || slot == kSlotRsiLoss ? PMENV_IND_RSI
         : slot == kSlotDxPlus || slot == kSlotDxMinus || slot == kSlotDxTr ? PMENV_IND_DX
         : slot == kSlotAdxPlus || slot == kSlotAdxMinus || slot == kSlotAdxTr || slot == kSlotAdx ? PMENV_IND_ADX
         : slot == kSlotObv ? PMENV_IND_OBV
         : PMENV_IND_ADOSC;
}

// kinds with a level-2 recurrence
constexpr unsigned kIndLevel2Mask = (1u << PMENV_IND_MACD) | (1u << PMENV_IND_ADX) | (1u << PMENV_IND_ADOSC);

// ---- the split form's geometry and the rule between the forms.
// One lane per column walks the whole series (ind_scan_seq_kernel): ceil(N / 64) waves. The
// split form cuts the rows behind the lookback into segments of kIndSegRows rows or more, at
// most kIndMaxSegs of them, and costs three walks of the bars instead of one; it pays while
// the sequential form leaves most of the chip idle.
constexpr int kIndSegRows = 32;
constexpr int kIndMaxSegs = 64;
// Columns up to which the split form is taken. MEASURED CROSSOVER (MI355X, the eight
// recurrence ops at T = 5,000, tools/bench_indicators.py, profiles/rows_indicators.json):
// the sequential form takes 8.0 - 8.3 ms from 510 to 16,384 columns (one walk's latency,
// whatever the columns), the split form 0.57 ms at 510, 2.5 ms at 8,192, 4.7 ms at 16,384
// and 9.6 ms at 32,768, where the sequential form takes 9.0 ms: the forms cross between
// 16,384 and 32,768 columns.
constexpr int kIndSplitMaxCols = 16384;

enum IndForm { kIndSeq = 0, kIndSplit = 1 };

struct IndOpInfo {
    int n_out = 0, lookback = 0;
    unsigned need = 0;          // channel bits
    bool scan = false;          // a recurrence (a walk) — otherwise windowed
    int p[3] = {0, 0, 0};       // normalised periods (MACD: fast <= slow)
};

inline bool ind_period_ok(int p) { return p >= 2 && p <= kIndMaxPeriod; }

// validates one op; PMENV_ERR_ARG for an unknown kind or a period outside 2 .. 256 (a
// band multiplier that is not finite likewise)
inline int ind_op_info(const pmenv_ind_op& op, IndOpInfo* o) {
    IndOpInfo r;
    const int a = op.p[0], b = op.p[1], c = op.p[2];
    switch (op.kind) {
    case PMENV_IND_EMA:
        if (!ind_period_ok(a)) return PMENV_ERR_ARG;
        r.n_out = 1; r.lookback = a - 1; r.need = kIndC; r.scan = true; r.p[0] = a;
        break;
    case PMENV_IND_BBANDS:
        if (!ind_period_ok(a) || !(op.f[0] - op.f[0] == 0.0) || !(op.f[1] - op.f[1] == 0.0)) return PMENV_ERR_ARG;
        r.n_out = 3; r.lookback = a - 1; r.need = kIndC; r.p[0] = a;
        break;
    case PMENV_IND_MACD:
        if (!ind_period_ok(a) || !ind_period_ok(b) || !ind_period_ok(c)) return PMENV_ERR_ARG;
        r.p[0] = a < b ? a : b; r.p[1] = a < b ? b : a; r.p[2] = c;      // swap if slow < fast
        r.n_out = 3; r.lookback = (r.p[1] - 1) + (c - 1); r.need = kIndC; r.scan = true;
        break;
    case PMENV_IND_ATR:
        if (!ind_period_ok(a)) return PMENV_ERR_ARG;
        r.n_out = 1; r.lookback = a; r.need = kIndH | kIndL | kIndC; r.scan = true; r.p[0] = a;
        break;
    case PMENV_IND_RSI:
        if (!ind_period_ok(a)) return PMENV_ERR_ARG;
        r.n_out = 1; r.lookback = a; r.need = kIndC; r.scan = true; r.p[0] = a;
        break;
    case PMENV_IND_ADX:
        if (!ind_period_ok(a)) return PMENV_ERR_ARG;
        r.n_out = 1; r.lookback = 2 * a - 1; r.need = kIndH | kIndL | kIndC; r.scan = true; r.p[0] = a;
        break;
    case PMENV_IND_DX:
        if (!ind_period_ok(a)) return PMENV_ERR_ARG;
        r.n_out = 1; r.lookback = a; r.need = kIndH | kIndL | kIndC; r.scan = true; r.p[0] = a;
        break;
    case PMENV_IND_STOCH:
        if (!ind_period_ok(a) || !ind_period_ok(b) || !ind_period_ok(c)) return PMENV_ERR_ARG;
        r.n_out = 2; r.lookback = (a - 1) + (b - 1) + (c - 1); r.need = kIndH | kIndL | kIndC;
        r.p[0] = a; r.p[1] = b; r.p[2] = c;
        break;
    case PMENV_IND_CCI:
        if (!ind_period_ok(a)) return PMENV_ERR_ARG;
        r.n_out = 1; r.lookback = a - 1; r.need = kIndH | kIndL | kIndC; r.p[0] = a;
        break;
    case PMENV_IND_OBV:
        r.n_out = 1; r.lookback = 0; r.need = kIndC | kIndV; r.scan = true;
        break;
    case PMENV_IND_ADOSC:
        if (!ind_period_ok(a) || !ind_period_ok(b)) return PMENV_ERR_ARG;
        r.n_out = 1; r.lookback = (a > b ? a : b) - 1; r.need = kIndH | kIndL | kIndC | kIndV; r.scan = true;
        r.p[0] = a; r.p[1] = b;
        break;
    default:
        return PMENV_ERR_ARG;
    }
    *o = r;
    return PMENV_OK;
}

// pmenv_ind_layout: K = the outputs of all ops in order, L = the largest lookback
inline int ind_layout(const pmenv_ind_op* ops, int32_t n_ops, int32_t* n_out, int32_t* lookback) {
    if (!ops || n_ops < 1 || n_ops > kIndMaxOps) return PMENV_ERR_ARG;
    int K = 0, L = 0;
    for (int i = 0; i < n_ops; ++i) {
        IndOpInfo o;
        if (ind_op_info(ops[i], &o) != PMENV_OK) return PMENV_ERR_ARG;
        K += o.n_out;
        L = o.lookback > L ? o.lookback : L;
    }
    if (n_out) *n_out = K;
    if (lookback) *lookback = L;
    return PMENV_OK;
}

// One walk of the bars: at most one op of each recurrence kind (each kind's state has its
// own registers); a second op of a kind opens a second walk.
struct IndWalk {
    unsigned mask = 0;                  // kinds present, 1 << kind
    unsigned need = 0;                  // channel bits
    int p[kIndKinds][3] = {};           // the kind's periods
    int col[kIndKinds] = {};            // the kind's first output column within the call's K
};

struct IndWindowOp {
    int kind = 0, col = 0;
    int p[3] = {0, 0, 0};
    double f[2] = {0.0, 0.0};
};

struct IndPlan {
    bool ok = false;
    int K = 0, L = 0;
    unsigned need = 0;
    int form = kIndSeq;
    int n_walks = 0;
    IndWalk walk[kIndMaxOps];
    int n_window = 0;
    IndWindowOp window[kIndMaxOps];
    bool stoch = false;                 // a fastk stream [T, N] f64 in the workspace
    // the split form: segment 0 is rows [0, L + seg_len), segment j >= 1 rows
    // [L + j * seg_len, L + (j + 1) * seg_len) cut at T
    int seg_len = 0, n_seg = 0;
    unsigned scan_grid = 0;             // column groups of 64 lanes
    unsigned window_grid = 0;           // blocks of kIndWindowBlock (row, column) pairs, output rows
    unsigned fastk_grid = 0;            // likewise over all T rows
    size_t rec_bytes = 0;               // split records [n_seg, kIndSlots, N] f64
    size_t fastk_off = 0;               // byte offset of the fastk stream
    size_t work_bytes = 0;
};

// force: -1 the rule below, kIndSeq / kIndSplit a tools build's override (split still needs
// two segments). Refused (ok = false): a bad op list, T <= L, N < 1, grids beyond 2^31 - 1.
inline IndPlan ind_plan(int32_t T, int32_t N, const pmenv_ind_op* ops, int32_t n_ops, int force = -1) {
    IndPlan p;
    int32_t K = 0, L = 0;
    if (ind_layout(ops, n_ops, &K, &L) != PMENV_OK || N < 1 || T <= L) return p;
    p.K = K;
    p.L = L;
    int seen[kIndKinds] = {};
    int col = 0;
    for (int i = 0; i < n_ops; ++i) {
        IndOpInfo o;
        ind_op_info(ops[i], &o);
        p.need |= o.need;
        const int k = ops[i].kind;
        if (o.scan) {
            IndWalk& w = p.walk[seen[k]];
            if (seen[k] + 1 > p.n_walks) p.n_walks = seen[k] + 1;
            ++seen[k];
            w.mask |= 1u << k;
            w.need |= o.need;
            for (int j = 0; j < 3; ++j) w.p[k][j] = o.p[j];
            w.col[k] = col;
        } else {
            IndWindowOp& w = p.window[p.n_window++];
            w.kind = k;
            w.col = col;
            for (int j = 0; j < 3; ++j) w.p[j] = o.p[j];
            w.f[0] = ops[i].f[0];
            w.f[1] = ops[i].f[1];
            if (k == PMENV_IND_STOCH) p.stoch = true;
        }
        col += o.n_out;
    }
    const int64_t R = (int64_t)T - L;
    const int64_t sg = ((int64_t)N + 63) / 64;
    const int64_t wg = (R * N + kIndWindowBlock - 1) / kIndWindowBlock;
    const int64_t fg = ((int64_t)T * N + kIndWindowBlock - 1) / kIndWindowBlock;
    if (sg > 0x7FFFFFFF || wg > 0x7FFFFFFF || fg > 0x7FFFFFFF) return p;
    p.scan_grid = (unsigned)sg;
    p.window_grid = (unsigned)wg;
    p.fastk_grid = (unsigned)fg;
    const bool can_split = p.n_walks > 0 && R >= 2 * (int64_t)kIndSegRows;
    const bool want_split = force < 0 ? N <= kIndSplitMaxCols : force == kIndSplit;
    if (can_split && want_split) {
        p.form = kIndSplit;
        int64_t len = (R + kIndMaxSegs - 1) / kIndMaxSegs;
        if (len < kIndSegRows) len = kIndSegRows;
        p.seg_len = (int)len;
        p.n_seg = (int)((R + len - 1) / len);
        p.rec_bytes = (size_t)p.n_seg * kIndSlots * (size_t)N * sizeof(double);
    }
    p.fastk_off = p.rec_bytes;
    p.work_bytes = p.rec_bytes + (p.stoch ? (size_t)T * (size_t)N * sizeof(double) : 0);
    p.ok = true;
    return p;
}

// a^n by n multiplications in ascending order (the split form's decay over one full
// segment; the same product on every host)
inline double ind_pow(double a, int n) {
    double r = 1.0;
    for (int i = 0; i < n; ++i) r *= a;
    return r;
}

// the coefficient a of a slot's recurrence s[t] = a * s[t-1] + b[t]
inline double ind_slot_coef(const IndWalk& w, int slot) {
    const int kind = ind_slot_kind(slot);
    const int* p = w.p[kind];
    switch (slot) {
    case kSlotEma: return 1.0 - 2.0 / (p[0] + 1);
    case kSlotMacdFast: return 1.0 - 2.0 / (p[0] + 1);
    case kSlotMacdSlow: return 1.0 - 2.0 / (p[1] + 1);
    case kSlotMacdSignal: return 1.0 - 2.0 / (p[2] + 1);
    case kSlotAtr: case kSlotRsiGain: case kSlotRsiLoss: case kSlotAdx: return (double)(p[0] - 1) / p[0];
    case kSlotDxPlus: case kSlotDxMinus: case kSlotDxTr:
    case kSlotAdxPlus: case kSlotAdxMinus: case kSlotAdxTr: return 1.0 - 1.0 / p[0];
    case kSlotAdFast: return 1.0 - 2.0 / (p[0] + 1);
    case kSlotAdSlow: return 1.0 - 2.0 / (p[1] + 1);
    default: return 1.0;                 // the running sums
    }
}

// pmenv_ind_path's string: the kernels of the call in launch order, " | " between them
inline void ind_plan_describe(const IndPlan& p, char* out, size_t size) {
    if (size) out[0] = 0;
    if (!p.ok) return;
    size_t n = 0;
    auto put = [&](const char* s) {
        const int k = snprintf(out + n, n < size ? size - n : 0, "%s%s", n ? " | " : "", s);
        if (k > 0) n += (size_t)k;
        if (n >= size) n = size - 1;
    };
    char buf[160];
    if (p.n_walks > 0) {
        if (p.form == kIndSplit)
            snprintf(buf, sizeof(buf), "ind_scan_split_kernel walks=%d seg=%d segs=%d grid=%ux%d block=64", p.n_walks,
                     p.seg_len, p.n_seg, p.scan_grid, p.n_seg);
        else
            snprintf(buf, sizeof(buf), "ind_scan_seq_kernel walks=%d grid=%u block=64", p.n_walks, p.scan_grid);
        put(buf);
    }
    if (p.stoch) {
        snprintf(buf, sizeof(buf), "ind_fastk_kernel grid=%u block=%d", p.fastk_grid, kIndWindowBlock);
        put(buf);
    }
    if (p.n_window > 0) {
        snprintf(buf, sizeof(buf), "ind_window_kernel ops=%d grid=%u block=%d", p.n_window, p.window_grid,
                 kIndWindowBlock);
        put(buf);
    }
}

}  // namespace pmenv_host
