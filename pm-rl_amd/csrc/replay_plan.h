// replay_plan.h — which kernel, and in which geometry, each sample gather launches:
// pmenv_replay_gather, pmenv_replay_gather_nstep, pmenv_replay_gather_seq and
// pmenv_rollout_gather switch on replay_plan(), pmenv_replay_path names its answer, and the
// tools build's replay hook takes replay_group() from here. Host only and pure: every
// decision is a function of integers, this header includes no HIP header and makes no HIP
// call (it compiles with a plain host compiler), and all products are taken in int64.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include "../../include/pmenv.h"

namespace pmenv_host {

enum ReplayForm {
    kReplayInvalid,   // a grid beyond 2^31 - 1 workgroups, or an unknown kind
    kReplayF5p,       // F = 5, persistent workgroups over asset groups staged in LDS (replay_*_f5p_kernel)
    kReplayLds,       // one workgroup per sample, the whole sample's days staged in LDS (replay_*_lds_kernel)
    kReplayElem,      // one thread per output float (replay_gather_kernel, replay_nstep_kernel, replay_seq_kernel)
    kRolloutTile,     // rollout_gather_tile_kernel: one workgroup per sample, staged in LDS
    kRolloutRows      // rollout_gather_rows_kernel: one wave per (sample, asset) row
};

constexpr int kReplayOutAligned = 1, kReplaySeriesAligned = 2;   // the `aligned` bits: 16-B aligned outputs / series

struct ReplayPlan {
    ReplayForm form = kReplayInvalid;
    int R = 0, gy = 0;               // f5p: asset rows per group, groups per sample (N / R)
    int D = 0;                       // f5p, LDS: staged days (W + 1, W + min(n, W), W + Lc)
    int ppt = 0;                     // f5p: (day, asset) pairs per thread
    int Lc = 0, nc = 0, items = 0;   // sequence f5p: elements per chunk, chunks per sequence, S * gy * nc
    int policy = 0;                  // f5p, tile: the window stores' cache-policy bits (0 plain, 2 nt, 16 sc1)
    unsigned grid_x = 0, grid_y = 1, block = 256;
    size_t lds_bytes = 0;
};

// F = 5 vector staging over asset groups of R rows: the largest R <= 256 that divides N with
// R*W*F a multiple of 4 (16-B aligned groups), at most max_pairs (day, asset) pairs over D
// staged days and an image of R*D*F + extra_floats floats within max_image_bytes; 0 where
// no group fits. The largest group: whole samples measured faster than 10-asset groups (131
// vs 148 us at N = 30, W = 50) — every workgroup pays the sample's dependent index loads
// once. N = 30, W = 50: R = 30, one group per sample.
inline int replay_group(int N, int W, int F, int64_t D, int64_t max_pairs, int64_t max_image_bytes,
                        int64_t extra_floats) {
    for (int r = N < 256 ? N : 256; r >= 1; --r)
        if (N % r == 0 && ((int64_t)r * W * F) % 4 == 0 && r * D <= max_pairs &&
            (r * D * F + extra_floats) * (int64_t)sizeof(float) <= max_image_bytes)
            return r;
    return 0;
}

// (day, asset) pairs per thread of a 256-thread workgroup: 2, 4, 8, then `top` (8 or 12)
inline int replay_ppt(int64_t pairs, int top) {
    for (int ppt = 2; ppt < top && ppt <= 8; ppt *= 2)
        if (pairs <= ppt * 256) return ppt;
    return top;
}

// the f5p forms of the one-step and the n-step gather: one workgroup per CU over groups of
// R rows and D staged days
inline void replay_plan_f5p(ReplayPlan& p, int N, int F, int S, int cus, int R, int D, int top_ppt) {
    p.form = kReplayF5p;
    p.R = R;
    p.D = D;
    p.gy = N / R;
    p.ppt = replay_ppt((int64_t)R * D, top_ppt);
    // s / s' are written once per sample: nt stores, 129.6 -> 118.6 us at S = 8,192
    // (tools/ab_replay.py, profiles/ab_r01/replay_nt_tpb_r01h.log). Persistent form
    // (replay_gather_f5p_kernel): one workgroup per CU loops over the samples with the
    // next sample's loads in flight. One per CU is the measured optimum (S = 8,192:
    // 96 us at 256 workgroups; 114-121 us at 192, 288, 512, 768, 1,280 and one
    // workgroup per sample, 117 us; profiles/ab_r01/replay_grid_r01j.log).
    p.policy = 2;
    const int G = cus / p.gy > 0 ? cus / p.gy : 1;
    p.grid_x = (unsigned)(S < G ? S : G);
    p.grid_y = (unsigned)p.gy;
    p.lds_bytes = (size_t)R * D * F * sizeof(float);
}

// the forms the one-step and the n-step gather share below the f5p form: one workgroup per
// sample with the D staged days in LDS when they fit in 64 KiB (16-B aligned outputs,
// N <= 256), else one thread per output float
inline void replay_plan_generic(ReplayPlan& p, int N, int F, int W, int S, int aligned, int D) {
    const int64_t lds = (int64_t)N * D * F * (int64_t)sizeof(float);
    if (lds <= 64 * 1024 && N <= 256 && (aligned & kReplayOutAligned)) {
        p.form = kReplayLds;
        p.D = D;
        p.grid_x = (unsigned)S;
        p.lds_bytes = (size_t)lds;
    } else {
        const int64_t threads = (int64_t)S * N * W * F;
        p.form = kReplayElem;
        p.grid_x = (unsigned)((threads + 255) / 256);
    }
}

// pmenv_replay_gather. F = 5: vector staging per asset group (replay_gather_f5p_kernel,
// persistent; or replay_gather_f5_kernel, one workgroup per sample: the tools build's);
// otherwise one workgroup per sample with the W+1 staged days in LDS when they fit in
// 64 KiB, else one thread per output float. Measured at S = 8,192, N = 30, W = 50: 96-102 us
// for the persistent f5 form, 117 us one workgroup per sample, 204 us for the per-element
// staging (tools/ab_replay.py, bench_rows.py)
inline ReplayPlan replay_plan_one_step(int N, int F, int W, int S, int aligned, int cus) {
    ReplayPlan p;
    const int D = W + 1;
    // R*(W+1) <= 2,048 (day, asset) pairs (at most 8 per thread), an image of 40 KiB at the most
    const int R = F == 5 && aligned == (kReplayOutAligned | kReplaySeriesAligned)
                      ? replay_group(N, W, F, D, 2048, 64 * 1024, 0) : 0;
    if (R > 0) replay_plan_f5p(p, N, F, S, cus, R, D, 8);
    else replay_plan_generic(p, N, F, W, S, aligned, D);
    return p;
}

// pmenv_replay_gather_nstep. The staged image holds the union of two overlapping windows:
// W + min(n, W) days. Same forms and the same asset-group rule as pmenv_replay_gather with
// that image: R divides N, R*W*F is a multiple of 4, at most 12 (day, asset) pairs per thread
// (N = 30, W = 50 keeps whole samples up to the disjoint case, 3,000 pairs), the
// image within 64 KiB. Measured at config 3's shape (S = 8,192, N = 30, W = 50) beside
// the one-step gather's 97 us: 122 us at n = 1, 126 us at n = 5, 245 us at n = 64
// (tools/bench_rows.py, profiles/rows_nstep.json). The generic LDS form has the
// one-step generic form's structure, which runs 198 us there: slower than the fast
// form at n <= 5 already on the one-step figure, and not timed at n = 64.
inline ReplayPlan replay_plan_nstep(int N, int F, int W, int n, int S, int aligned, int cus) {
    ReplayPlan p;
    const int D = W + (n < W ? n : W);
    const int R = F == 5 && aligned == (kReplayOutAligned | kReplaySeriesAligned)
                      ? replay_group(N, W, F, D, 12 * 256, 64 * 1024, 0) : 0;
    if (R > 0) replay_plan_f5p(p, N, F, S, cus, R, D, 12);   // one workgroup per CU, as the one-step gather
    else replay_plan_generic(p, N, F, W, S, aligned, D);
    return p;
}

// pmenv_replay_gather_seq; policy < 0 and lc_knob = 0: the product's rules (the tools build
// sets them, pmenv_tools::replay_seq_knobs).
// F = 5 fast form (replay_seq_f5p_kernel): asset groups of R rows by the n-step rule — R
// divides N, R*W*F is a multiple of 4, at most 12 (day, asset) pairs per thread, the
// image [R][W + Lc][5] (+16 B) within 64 KiB — sized so that a chunk holds min(L, 8)
// elements, or one where no group does. Lc, the elements per chunk: 8 where the image
// holds them, fewer where that leaves a CU without an item (Dreamer's 16 sequences of 64
// elements: 4). Measured on config 3's ring: 128 x 64 (nt stores) takes 69 us at Lc = 4
// and 8, 72-73 us at 16 and 32, 98 us at 2, 159 us at 1; 16 x 64 (sc1 stores) takes
// 10.0 us at 4, 13.4-14.0 us at 2 and 8, 21-37 us at 1, 16 and 32 (tools/bench_rows.py's
// PMENV_SEQ_LC rows, profiles/rows_seq_ab.json).
inline ReplayPlan replay_plan_seq(int N, int F, int W, int L, int S, int aligned, int cus, int policy,
                                  int lc_knob) {
    ReplayPlan p;
    auto group = [&](int lc) { return replay_group(N, W, F, (int64_t)W + lc, 12 * 256, 64 * 1024, 4); };
    int R = 0;
    if (F == 5 && aligned == (kReplayOutAligned | kReplaySeriesAligned)) {
        R = group(L < 8 ? L : 8);
        if (!R) R = group(1);
    }
    const int gy = R ? N / R : 1;
    if (R > 0 && (int64_t)S * gy * L <= (1 << 30)) {
        int64_t cap = 12 * 256 / R;
        if (cap > (64 * 1024 / 4 - 4) / (F * R)) cap = (64 * 1024 / 4 - 4) / (F * R);
        cap -= W;
        if (cap > 256) cap = 256;
        if (cap > L) cap = L;
        int64_t nc = (L + (cap < 8 ? cap : 8) - 1) / (cap < 8 ? cap : 8);
        const int64_t want = ((int64_t)cus + (int64_t)S * gy - 1) / ((int64_t)S * gy);   // chunks for an item a CU
        if (nc < want) nc = want < L ? want : L;
        int Lc = (int)((L + nc - 1) / nc);
        if (lc_knob > 0) Lc = (int)(lc_knob < cap ? lc_knob : cap);
        nc = (L + Lc - 1) / Lc;
        p.form = kReplayF5p;
        p.R = R;
        p.gy = gy;
        p.Lc = Lc;
        p.nc = (int)nc;
        p.items = (int)((int64_t)S * gy * nc);
        p.D = W + Lc;
        p.ppt = replay_ppt((int64_t)R * p.D, 12);
        p.lds_bytes = ((size_t)R * p.D * F + 4) * sizeof(float);
        // the windows are written once and read by the learner later: the rollout gather's
        // rule — sc1 stores while they fit the Infinity Cache, nt stores above — with the
        // bound where this kernel was measured: 31 MB (16 x 64) 21.7 us sc1, 23.2 nt, 24.4
        // plain; 245 MB (128 x 64) 50.7 us sc1, 57.2 plain, 69.0 nt (PMENV_SEQ_NT rows,
        // profiles/rows_seq_ab.json). Above 256 MiB nothing was measured for this kernel:
        // nt, as the rollout gather's sc1 loses there
        if (policy < 0) policy = (int64_t)S * L * N * W * F * (int64_t)sizeof(float) <= ((int64_t)256 << 20) ? 16 : 2;
        p.policy = policy == 16 || policy == 2 ? policy : 0;
        p.grid_x = (unsigned)(p.items < cus ? p.items : cus);
    } else {
        const int64_t threads = (int64_t)S * L * N * W * F;
        const int64_t blocks = (threads + 255) / 256;
        if (blocks > 0x7FFFFFFF) return p;
        p.form = kReplayElem;
        p.grid_x = (unsigned)blocks;
    }
    return p;
}

// pmenv_rollout_gather and pmenv_rollout_gather_env
inline ReplayPlan replay_plan_rollout(int N, int F, int W, int S, int aligned) {
    ReplayPlan p;
    const int64_t lds = (int64_t)W * N * F * (int64_t)sizeof(float);
    // market [W][N][4] + weights [W][N]; the tile's 16-B series loads and window stores need
    // 16-B aligned series / s (C callers may pass sliced views: those take the row form)
    const bool tile = F == 5 && ((int64_t)N * W * F) % 4 == 0 && lds <= 64 * 1024 &&
                      aligned == (kReplayOutAligned | kReplaySeriesAligned);
    // the windows are written once and read by the learner later: nt stores (the tile's
    // bits unchanged), per call 29.0 -> 27.5 us at 4,096 samples, 235.1 -> 196.9 at 32,768,
    // 74.4 -> 54.3 at 8,192 from a 65,536 x 64 buffer; windows that fit well inside the
    // Infinity Cache (<= 128 MiB) take sc1 stores instead: 24.1-24.5 us at 4,096 samples
    // (123 MB), which lose 1.5-2x from 245 MB up (profiles/rows_r03ad/, rows_r03ae/)
    if (tile) {                                            // one workgroup per sample, staged in LDS
        const bool small = (int64_t)S * N * W * F * (int64_t)sizeof(float) <= ((int64_t)128 << 20);
        p.form = kRolloutTile;
        p.policy = small ? 16 : 2;
        p.grid_x = (unsigned)S;
        p.lds_bytes = (size_t)lds;
    } else {
        const int64_t rows = (int64_t)S * N;               // one wave per (sample, asset) row
        p.form = kRolloutRows;
        p.grid_x = (unsigned)((rows + 3) / 4);
    }
    return p;
}

// The one place that decides which kernel a sample gather takes. kind: pmenv_replay_kind;
// n: the n-step gather's n or the sequence gather's L; aligned: kReplayOutAligned |
// kReplaySeriesAligned; cus: the device's compute units; policy, lc_knob: the sequence
// gather's tools knobs (-1, 0 in the product).
inline ReplayPlan replay_plan(int kind, int N, int F, int W, int n, int S, int aligned, int cus, int policy = -1,
                              int lc_knob = 0) {
    switch (kind) {
    case PMENV_REPLAY_ONE_STEP: return replay_plan_one_step(N, F, W, S, aligned, cus);
    case PMENV_REPLAY_NSTEP: return replay_plan_nstep(N, F, W, n, S, aligned, cus);
    case PMENV_REPLAY_SEQ: return replay_plan_seq(N, F, W, n, S, aligned, cus, policy, lc_knob);
    case PMENV_REPLAY_ROLLOUT: return replay_plan_rollout(N, F, W, S, aligned);
    default: return ReplayPlan();
    }
}

// pmenv_replay_path's string for a plan: the kernel as the library instantiates it, then
// R, the staged days and the sequence chunks where the form has them, the grid and the LDS bytes.
// env: the rollout forms' per-env kernels (pmenv_rollout_gather_env: the same plan)
inline void replay_plan_describe(int kind, const ReplayPlan& p, char* out, size_t size, bool env = false) {
    static const char* const stem[] = {"replay_gather", "replay_nstep", "replay_seq"};
    char name[64] = "";
    if (size) out[0] = 0;
    switch (p.form) {
    case kReplayF5p: snprintf(name, sizeof(name), "%s_f5p_kernel<%d,%d>", stem[kind], p.ppt, p.policy); break;
    case kReplayLds: snprintf(name, sizeof(name), "%s_lds_kernel", stem[kind]); break;
    case kReplayElem: snprintf(name, sizeof(name), "%s_kernel", stem[kind]); break;
    case kRolloutTile:
        snprintf(name, sizeof(name), "rollout_gather_%stile_kernel<%d>", env ? "env_" : "", p.policy);
        break;
    case kRolloutRows: snprintf(name, sizeof(name), "rollout_gather_%srows_kernel", env ? "env_" : ""); break;
    default: return;
    }
    int at = snprintf(out, size, "%s R=%d", name, p.R);
    if (p.D && at < (int)size) at += snprintf(out + at, size - at, " D=%d", p.D);
    if (p.Lc && at < (int)size) at += snprintf(out + at, size - at, " Lc=%d nc=%d", p.Lc, p.nc);
    if (at < (int)size) snprintf(out + at, size - at, " grid=%ux%u lds=%zu", p.grid_x, p.grid_y, p.lds_bytes);
}

}  // namespace pmenv_host
