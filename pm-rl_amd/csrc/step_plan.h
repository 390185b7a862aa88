// step_plan.h — which kernel an advance or surface step launches, and in which geometry:
// everything of the handle that is a pure function of pmenv_cfg. pmenv_create_in runs
// step_plan() and step_plan_finish() (the tools build's plan hook between them),
// pmenv_set_step_path is step_plan_select(), pmenv_step_ex switches on step_route(), and
// pmenv_step_path / pmenv_step_path_for format the plan with step_plan_describe(). The host
// constants the plan and the kernels share are defined here, once; common.h includes this
// header for them. Host only and pure: every decision is a function of integers (and the
// commission's sign), this header includes no HIP header and makes no HIP call (it compiles
// with a plain host compiler), reads no environment variable, and takes every product in int64.
#pragma once

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/pmenv.h"

namespace pmenv_dev {

constexpr int kWideMaxAssets = 512;   // the widest env the packed scalar step and the wide flat step take
constexpr int kBlock = 256;         // threads per env workgroup (LDS / surface / reset kernels)
constexpr int kMaxVec = 8;          // float4 per thread for one LDS tile
constexpr int kTileFloats = kBlock * kMaxVec * 4;  // 8192 floats = 32 KiB LDS tile
constexpr int kScalarWaves = 4;     // envs (waves) per scalar_step_kernel workgroup
constexpr int kStreamBlock = 512;   // threads per advance_rows_kernel workgroup

// bytes of the per-env scalar scratch (env_step.h: Scratch) behind a tile of tile_floats floats
inline size_t scratch_bytes(int tile_floats, int N, int F) {
    return (size_t)tile_floats * 4 + (size_t)N * 16 + (size_t)N * 8 + (size_t)N * (F - 1) * 4 + 16;
}

}  // namespace pmenv_dev

namespace pmenv_host {

constexpr int PMENV_FUSE_DB = 1, PMENV_FUSE_INPLACE = 2;
constexpr int kOneV = 4;              // step_env_kernel: 16-B chunks per lane
constexpr int kK1Str = 100000;        // k1_vec: the strided layout of scalar_step_vec_kernel

// The shape plan: fixed once pmenv_create_in returns, but for the current selection (path,
// one, flat1, relay, gen), which pmenv_set_step_path rewrites through step_plan_select.
struct StepPlan {
    // the register step (step_small_kernel<small_block, small_e>): any F, any alignment, env
    // windows of at most 1,024 x 16 floats; 0: the LDS fallback
    int small_block, small_e;
    bool tiny;            // ... of at most 256 x 8 floats and N <= 64: step_tiny_kernel (LDS-staged)
    bool surf_stream;     // surface steps as two launches: the scalar step, then surface_stream_kernel
    size_t surf_lds;      // its workgroup's rows' ring columns (rows x W floats)
    // LDS single-launch fallback geometry
    int rows_per_tile, tile_floats;
    bool vec;
    size_t lds_tile, lds_surface;
    // two-launch path: the scalar step, then the window stream
    bool streaming;       // F = 5, 16-B granular env windows: the streams below apply
    int unit_rows, units_per_env, stream_vec;          // row-kernel advance in place
    int unit_rows_db, units_per_env_db, stream_vec_db; // row-kernel advance double-buffered (obs_out)
    bool flat_ok;         // the flat 16-B stream's shape rules hold
    bool flat;            // double-buffered advance as the flat 16-B stream
    int flat_pol, flat_ip_pol;   // cache policy (0 default, 1 nt): double-buffered / in-place stream
    bool flat_inplace;    // in-place advance as the flat stream + halo (advance_flat_inplace_kernel)
    int flat_ip_block, flat_ip_vec;   // threads per workgroup, chunks per thread
    uint32_t halo_wgs, flat_qtot;
    size_t halo_bytes;    // [halo_wgs + 1][2] float4 (four past F = 8): the in-place stream's halo; 0: none
    int scalar_scratch_floats;
    size_t lds_scalar;
    // two-launch path for F != 5 (2 <= F <= 8, 16-B granular env windows): the scalar step,
    // then the generic stream (advance_gen_kernel<gen_block, gen_v>)
    bool gen_ok;          // the shape fits the generic stream
    int gen_auto;         // PMENV_FUSE_* bits the automatic choice gives it
    int gen;              // PMENV_FUSE_* bits: which windows take it now
    int gen_block, gen_v; // threads per workgroup, chunks per thread
    uint32_t gen_qtot;    // chunks of the whole [B, N, W, F] window
    int k1_vec;           // scalar_step_vec_kernel shape 100 * L + A (+ kK1Str), 0: register / LDS form
    // one launch per step, one workgroup per env (step_env_kernel)
    bool one_ok;          // the shape fits step_env_kernel
    int one_auto;         // PMENV_FUSE_* bits the automatic choice gives step_env_kernel
    int one;              // PMENV_FUSE_* bits: which windows take step_env_kernel now
    int one_waves;        // waves per workgroup
    uint32_t per4;        // 16-B chunks per env window
    // one launch over the flat stream (step_flat_kernel / step_flat_vec_kernel)
    bool flat1_ok;        // the shape fits the flat one-launch step
    int flat1_auto;       // PMENV_FUSE_* bits the automatic choice gives it
    int flat1;            // PMENV_FUSE_* bits: which windows take it now
    int flat1_block, flat1_vec;   // threads per workgroup, chunks per thread
    uint32_t halo1_wgs;
    // the snapshot allocation (flat1_ok): two parities of state_b + halo_b, then the 64 B of seq
    size_t snap_state_bytes;   // one parity: value f64 | counter i32 | get_last() | last close, 16-B aligned fields
    size_t snap_halo_bytes;    // one parity's tile halo: [halo1_wgs + 1][2] float4
    size_t snap_bytes;
    // one launch, scalar blocks relaying w' and the counter to the stream tiles (step_relay.h)
    bool relay_ok;        // the shape fits step_relay_kernel
    int relay_auto;       // PMENV_FUSE_* bits the automatic choice gives it
    int relay;            // PMENV_FUSE_* bits: which windows take it now
    int relay_kl, relay_ka;   // the scalar step's form: KL lanes per env, KA strided assets per lane (0: register)
    int relay_block, relay_v; // the tiles' geometry: relay_block threads x relay_v 16-B chunks
    int relay_epb;        // envs per scalar block (relay_block / 64 waves x 64 / relay_kl envs)
    uint32_t relay_tiles, relay_scal;
    // the relay allocation (relay_ok): 64 B of control words | words_b | kp_b x 2 | halo_b x 2
    size_t relay_words_bytes;  // the relay words [B * N] {epoch, w'}, 16-B padded, then the deferral list and claims
    size_t relay_kp_bytes;     // one parity's counter copy
    size_t relay_halo_bytes;   // one parity's tile halo
    size_t relay_bytes;
    int path;             // pmenv_step_path_kind
};

// the message into err (where given), PMENV_ERR_ARG back
__attribute__((format(printf, 3, 4))) inline int plan_err(char* err, size_t err_len, const char* fmt, ...) {
    if (err && err_len) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, err_len, fmt, ap);
        va_end(ap);
    }
    return PMENV_ERR_ARG;
}

inline size_t up16(size_t x) { return (x + 15) / 16 * 16; }

// saturates where the product passes int64 (B N W F beyond 2^61: shapes step_plan_finish
// refuses for their LDS), so every threshold below compares as for the true size
inline int64_t window_bytes(const pmenv_cfg& c) {
    const int64_t per = (int64_t)c.num_assets * c.window * c.features;
    const int64_t lim = INT64_MAX / 4;
    return per > 0 && c.num_envs > lim / per ? INT64_MAX : (int64_t)c.num_envs * per * 4;
}

// K1 shape per asset count: N <= 64 keeps one asset per lane, with reductions bitwise
// those of the one-launch steps' scalar part (so the paths, and sharded and unsharded
// runs whose path can differ by env count, give the same bits): N <= 16 the packed form
// with 8 / 16 lanes per env (8 / 4 envs per wave instead of 2; its butterfly pairs the
// lanes as the row shifts do, every pair sum commutes bitwise, and the all-zero padding
// lanes of the register form only add +0.0, which the packed form's 0.0 + x seed
// reproduces), 16 < N <= 64 the register form; 64 < N <= 512 the packed strided form
// (64 lanes x A assets, every dword load a coalesced run; step_flat_vec_kernel shares
// it); N > 512 the LDS form.
inline int pick_k1_vec(const pmenv_cfg& c) {
    const int N = c.num_assets;
    if ((int64_t)c.num_envs * N * 4 >= (1ll << 32)) return 0;     // descriptors span the [B*N] arrays
    if (N <= 8) return kK1Str + 801;
    if (N <= 16) return kK1Str + 1601;
    if (N <= 64) return 0;
    if (N <= 128) return kK1Str + 6402;
    if (N <= 256) return kK1Str + 6404;
    if (N <= 512) return kK1Str + 6408;
    return 0;
}

// Geometry of the row-kernel stream (the fallback of the flat stream): units of R whole
// asset rows per `block`-thread workgroup, R*W*F floats <= 4*block*V (V float4 per
// thread) and R*W*F % 4 == 0 so every unit starts 16-B aligned. `v_order` lists V in
// preference order; want_rows > 0 forces R (tools A/B). Returns false when the shape
// needs the LDS fallback.
inline bool plan_streaming(const pmenv_cfg& c, const int* v_order, int block, int want_rows, int* unit_rows,
                           int* vec_per_thread) {
    const int64_t WF = (int64_t)c.window * c.features;
    if (c.features != 5 || ((int64_t)c.num_assets * WF) % 4 != 0) return false;
    int align = 1;                       // rows per unit must be a multiple of this
    while ((align * WF) % 4 != 0) ++align;
    static const int kAscending[3] = {1, 2, 4};
    if (want_rows > 0) v_order = kAscending;   // a forced unit takes the fewest float4 per thread that hold it
    for (int vi = 0; vi < 3; ++vi) {
        const int V = v_order[vi];
        const int64_t cap = (int64_t)block * 4 * V;
        int R = (int)(cap / WF);
        if (R >= c.num_assets) R = c.num_assets;
        else R -= R % align;
        if (R < 1 || (int64_t)R * WF > cap) continue;
        if (want_rows > 0) {
            if (want_rows > R) continue;
            if (want_rows != c.num_assets && want_rows % align) return false;
            R = want_rows;
        }
        *unit_rows = R;
        *vec_per_thread = V;
        return true;
    }
    return false;
}

// The one-workgroup-per-env step with V chunks per lane: waves per workgroup and whether
// the shape fits (F = 5, W >= 2, N <= 64: the scalar step on one wave; the env's 1 KiB
// blocks in at most 16 waves and 64 KiB of LDS)
inline void plan_one(const pmenv_cfg& c, StepPlan& p, int V) {
    const int64_t per = (int64_t)c.num_assets * c.window * c.features;
    // the env's chunks start anywhere in a 64-chunk block: up to 63 slots ahead of it
    const uint32_t blocks = (p.per4 + 63u + 63u) / 64u;
    p.one_waves = (int)((blocks + (uint32_t)V - 1) / (uint32_t)V);
    p.one_ok = p.streaming && c.features == 5 && c.window >= 2 && c.num_assets <= 64 && per % 4 == 0 &&
               p.one_waves <= 16 && ((int64_t)64 * V * p.one_waves + 2) * 16 <= 65536;
}

// The flat one-launch step in `block` x `vec` tiles: the flat stream's shape rules, at
// most one env per wave in a tile, N <= 64 — or, for wide envs (64 < N <= 512,
// step_flat_vec_kernel), the rows a tile touches per env within one wave's 64 staged bar
// rows (W >= 14 at F = 5 for 16 KiB tiles)
inline bool flat1_fits(const pmenv_cfg& c, const StepPlan& p, int block, int vec) {
    const int64_t WF = (int64_t)c.window * c.features;
    const uint32_t cpw = (uint32_t)(block * vec);
    const uint32_t ne_max = p.per4 ? (cpw + p.per4 - 2u) / p.per4 + 1u : 0u;
    const int64_t span_rows = (4ll * cpw - 1) / (WF > 0 ? WF : 1) + 2;
    const bool wide_ok = c.num_assets <= pmenv_dev::kWideMaxAssets && span_rows <= 64;
    return p.flat_ok && (c.num_assets <= 64 || wide_ok) && ne_max <= (uint32_t)(block / 64);
}

// the relay step's deferral list ({epoch, count} + one entry per tile) and tile claims, 16-B padded
inline size_t relay_list_bytes(const StepPlan* p) {
    const size_t tiles = p->relay_tiles;
    return ((tiles + 1) * 8 + 15) / 16 * 16 + (tiles * 4 + 15) / 16 * 16;
}

// The argument checks of pmenv_create and the plan of every step path for the shape.
// PMENV_ERR_ARG with the message in err where pmenv_create refuses the cfg; step_plan_finish
// completes the plan (the tools build rewrites some of it in between).
inline int step_plan(const pmenv_cfg& c, StepPlan* plan, char* err, size_t err_len) {
    using namespace pmenv_dev;
    StepPlan& p = *plan;
    p = StepPlan();
    if (c.num_envs < 1 || c.num_assets < 1 || c.window < 1 || c.features < 2)
        return plan_err(err, err_len, "invalid shape B=%d N=%d W=%d F=%d (need B,N,W >= 1, F >= 2)", c.num_envs,
                        c.num_assets, c.window, c.features);
    if (c.close_channel < 0 || c.close_channel >= c.features - 1)
        return plan_err(err, err_len, "close_channel %d must be a market channel in [0, F-2]", c.close_channel);
    if (c.reward_kind < 0 || c.reward_kind > 3 || c.norm_mode < 0 || c.norm_mode > 1 || c.ring_mode < 0 ||
        c.ring_mode > 1 || c.ret_mode < 0 || c.ret_mode > 2 || c.mu_max_iter < 0 || !(c.commission >= 0.0) ||
        !(c.commission < 1.0))
        return plan_err(err, err_len, "invalid mode/commission value in cfg");
    const int64_t WF = (int64_t)c.window * c.features;
    if (WF > kTileFloats)
        return plan_err(err, err_len, "window*features = %lld exceeds the %d-float LDS tile", (long long)WF, kTileFloats);
    if ((int64_t)c.num_assets * WF >= (1ll << 31)) return plan_err(err, err_len, "per-env obs block too large");
    // LDS fallback tile geometry: whole asset rows, 16-B granular when every env block is
    int R = (int)(kTileFloats / WF);
    if (R > c.num_assets) R = c.num_assets;
    bool vec = ((int64_t)c.num_assets * WF) % 4 == 0;
    if (vec && R < c.num_assets) {
        while (R > 0 && ((int64_t)R * WF) % 4 != 0) --R;
        if (R == 0) { vec = false; R = (int)(kTileFloats / WF); }
    }
    p.rows_per_tile = R;
    p.vec = vec;
    // the register step: the env's window within BLOCK x E floats (one workgroup per env)
    {
        const int64_t nwf = (int64_t)c.num_assets * WF;
        p.small_block = nwf <= 256 * 16 ? 256 : nwf <= 512 * 16 ? 512 : nwf <= 1024 * 16 ? 1024 : 0;
        p.small_e = nwf <= 256 * 8 ? 8 : 16;
        // config 1's 1 x 5 x 50 x 5: 4.1 us (step_small_kernel) -> see DESIGN.md §3
        // (step_tiny_kernel stages the day's bar two floats per thread: N (F - 1) <= 2 x 256)
        p.tiny = p.small_block == 256 && p.small_e == 8 && c.num_assets <= 64 &&
                 (int64_t)c.num_assets * (c.features - 1) <= 2 * 256;
    }
    // surface steps on windows past the Infinity Cache with 16-B granular env blocks: the scalar
    // step, then surface_stream_kernel (65,536 x 30 x 50 x 5 723 us with the ring columns staged
    // in LDS, against 939 on the per-env kernel's dword writes, 892 with its writes in whole
    // chunks; cache-resident windows keep the per-env kernel: 4,096 x 30 38.3 against 48.6 in
    // whole chunks — ab_r05/surface_stream_r05s4_*, surface_ringlds_r05sr.*); the staged
    // columns (rows x W floats) and counters (rows) within 64 KiB
    p.surf_lds = (size_t)(4 * 1024 / WF + 2) * (c.window + 1) * 4;   // + each row's counter
    p.surf_stream = window_bytes(c) > (256ll << 20) && ((int64_t)c.num_assets * WF) % 4 == 0 &&
                    (int64_t)c.num_envs * ((int64_t)c.num_assets * WF / 4) < (1ll << 31) - 1024 &&
                    p.surf_lds <= (64u << 10) && 4 * 1024 / WF + 2 <= 256;   // a thread per row's counter
    p.tile_floats = (int)((((int64_t)R * WF) + 3) / 4 * 4);
    p.lds_tile = scratch_bytes(p.tile_floats, c.num_assets, c.features);
    p.lds_surface = scratch_bytes(0, c.num_assets, c.features);

    // ---- the two-launch stream: row-kernel geometry (fallback) and the flat stream
    static const int kInplaceOrder[3] = {2, 4, 1}, kDoubleOrder[3] = {4, 2, 1};
    p.streaming = plan_streaming(c, kInplaceOrder, kStreamBlock, 0, &p.unit_rows, &p.stream_vec) &&
                  plan_streaming(c, kDoubleOrder, kStreamBlock, 0, &p.unit_rows_db, &p.stream_vec_db);
    const int64_t per = (int64_t)c.num_assets * c.window * c.features;
    const int64_t win = window_bytes(c);
    // Flat 16-B stream (F = 5, W >= 2, 16-B granular envs, chunk count < 2^31) in place
    // (with the halo) and double-buffered: 512 threads x 2 chunks, side data through the
    // scalar unit (6.38 TB/s against 5.37 for whole-row units).
    p.flat_ok = p.streaming && c.features == 5 && c.window >= 2 && per % 4 == 0 &&
                (int64_t)c.num_envs * (per / 4) < (1ll << 31) - 1024;
    p.flat = p.flat_inplace = p.flat_ok;
    // in place, cache-resident windows (<= 256 MiB) take 8 KiB workgroups: 80.2 vs 83.2 us
    // at 8,192 x 30, 44.4 vs 44.7 at 4,096 (profiles/ab_r02/r02w_smallip_*); above, 16 KiB
    // (round 1: 512 x 2 against 256 x 1 / 2 / 4, 512 x 1, 1024 x 1)
    p.flat_ip_block = win <= (256ll << 20) ? 256 : 512;
    p.flat_ip_vec = 2;
    p.flat_qtot = p.flat_ok ? (uint32_t)((int64_t)c.num_envs * (per / 4)) : 0u;
    // nt unless the stream's working set fits the 256 MiB Infinity Cache: the window in
    // place (<= 256 MiB), the window and its double buffer otherwise (<= 128 MiB each).
    // Step at 4,096 x 30 x 50 x 5 (123 MB) 44.4 us with the default policy against 46.5
    // nt; 8,192 envs (246 MB) in place 84.6 / 86.1 but double-buffered 91.2 / 86.5;
    // 16,384: 199.6 / 164.6 (profiles/ab_r01/pol_small_r01j.log, pol_ip_r01m.log)
    p.flat_pol = win <= (128ll << 20) ? 0 : 1;
    p.flat_ip_pol = win <= (256ll << 20) ? 0 : 1;
    p.k1_vec = pick_k1_vec(c);
    p.per4 = (uint32_t)(per / 4);

    // ---- the one-launch step (step_env_kernel, one workgroup per env): F = 5, W >= 2,
    // N <= 64 (the scalar step on one wave), 16-B granular env windows whose 1 KiB
    // blocks fit 16 waves and 64 KiB of LDS, 4 chunks per lane (650 us against 662-666
    // for 8, 762 for 3, 860 for 2 at the BASELINE shape). AUTO gives it the windows of at
    // most 48 MiB, where launch latency dominates and it wins by 7-38 % (tools/gpu_ab_smallb.sh,
    // profiles/ab_r02/r02u_*: N = 8..64, 256..4,096 envs; N = 30: 64 envs 6.5 vs 9.6 us,
    // 1,024: 13.1 vs 18.2). Larger windows take the two-launch stream: its fixed 16 KiB
    // workgroups run 640-670 us on a 2 GB window at every asset count measured, while the
    // one-workgroup-per-env geometry ties it only at N = 30 (650-658 us) and loses 4-15 %
    // at N = 8, 16, 24, 32, 40, 48, 60, 64 (profiles/ab_r02/r02r_*, r02s_*, r02t_*).
    // (Also beyond the flat stream's 2^31-chunk index, where the two-launch path would
    // fall back to the whole-row stream.)
    plan_one(c, p, kOneV);
    p.one_auto = p.one_ok && (win <= (48ll << 20) || !p.flat_inplace) ? (PMENV_FUSE_DB | PMENV_FUSE_INPLACE) : 0;

    // ---- the one-launch flat step (step_flat_kernel; step_flat_vec_kernel for 64 < N <=
    // 512): the flat stream's shape rules, the scalar step on one wave per env, at most one
    // env per wave in a tile (flat1_fits). Geometry: 256 threads x 4 chunks (16 KiB tiles,
    // 4 waves) where env windows have >= 511 chunks, 512 x 2 (8 waves) from 148 chunks.
    // 256 x 4 against 512 x 2 / 512 x 4 / 1024 x 2 / 256 x 8 / 256 x 2 / 128 x 8 / 128 x 4 at
    // 65,536 x 30 in place: 629.5 against 714 / 678 / 790 / 695 / 675 / 624 / 641 us; 128 x 8
    // loses 15 % at N = 16 and 64 where 256 x 4 wins (profiles/ab_r02/r02w_flat1b_*,
    // r02w_flat1c_*). A persistent form that keeps the next tile's loads in flight needs
    // 160 VGPRs (3 waves per SIMD): 2x slower.
    // 128 x 8 (2 waves, 8 chunks per lane, the same 16 KiB tiles) where every tile holds at
    // most two envs (1,023 .. 1,999 chunks per env: N = 20 .. 39 at W = 50) and the window
    // streams through HBM: 0.5-1.1 % ahead of 256 x 4 from 49,152 envs at N = 30 (65,536:
    // 625.7 vs 629.4 and 628.8 vs 631.6 us; 98,304: 941.1 vs 951.6), N = 20 / 24 / 28 by
    // 1.0 / 0.7 / 0.5 %; behind it at 16,384 envs (162.9 vs 161.4) and at N = 16 / 64
    // (profiles/ab_r02/r02w_flat1k_*, r02w_flat1l_*, r02w_flat1c_*). Wide envs: 256 x 4.
    const bool band128 = c.num_assets <= 64 && p.per4 >= 1023u && p.per4 < 2000u && win > (1ll << 30);
    if (band128 && flat1_fits(c, p, 128, 8)) { p.flat1_block = 128; p.flat1_vec = 8; }
    else if (flat1_fits(c, p, 256, 4)) { p.flat1_block = 256; p.flat1_vec = 4; }
    else { p.flat1_block = 512; p.flat1_vec = 2; }
    p.flat1_ok = flat1_fits(c, p, p.flat1_block, p.flat1_vec) && (c.num_assets <= 64 || p.flat1_block == 256);
    // AUTO: above the one-launch-per-env windows (48 MiB) the flat step beats the two-launch
    // stream by 1-3.5 % for env windows of >= 1,000 chunks (N >= 16 at W = 50): 65,536 x 30
    // 629.5 / 639.7 against 642.4 / 648.8 us on two boxes, N = 24 / 40 / 48 / 64 by 1-3.4 %,
    // N = 16 681 vs 689; it loses at N = 8 (500 chunks, 4 envs per tile: 713 vs 691) and in
    // place on cache-resident windows (4,096 envs: 46.3 vs 44.2 us, 8,192: 85.2 vs 84.2);
    // double-buffered it wins from 2,048 envs (25.4 vs 27.0) (profiles/ab_r02/r02w_flat1d_*).
    // Commission > 0: every tile an env straddles runs the capped fixed point. With the
    // active-set iteration (scalar_core), a uniform wave index (no waterfall loops around
    // the scalar loads) and the reciprocal of 1 - c w0, the flat step leads there too:
    // 65,536 x 30 at 0.0025 642.8 vs 661.9 us on two launches (profiles/ab_r03/comm3_r03.err;
    // in round 2 the fixed point cost it 6-8 %: 701 vs 662).
    p.flat1_auto = 0;
    if (p.flat1_ok && c.num_assets <= 64 && p.flat1_block <= 256 && p.per4 >= 1000u) {
        if (win > (48ll << 20)) p.flat1_auto |= PMENV_FUSE_DB;
        if (win > (256ll << 20)) p.flat1_auto |= PMENV_FUSE_INPLACE;
        p.one_auto &= ~p.flat1_auto;
    }
    // Wide envs (step_flat_vec_kernel, 64 < N <= 512): every tile an env straddles runs the
    // env's whole packed scalar step, which costs more than the kernel boundary it saves
    // from 4 assets per lane on: 8,192 x 500 in place 1,512 (128 x 8) / 1,605 (256 x 4)
    // against 1,381 us on two launches, 2,048 x 200 143.5 vs 140.0; at 2 assets per lane
    // it wins on HBM-streamed windows: 16,384 x 100 532.9 vs 549.7 us (profiles/ab_r03/
    // wide_r03wide.err). AUTO gives it in-place windows > 1 GiB at N <= 128 without commission.
    if (p.flat1_ok && c.num_assets > 64 && c.num_assets <= 128 && win > (1ll << 30) && !(c.commission > 0.0))
        p.flat1_auto |= PMENV_FUSE_INPLACE;
    // In place, 24-100 MiB: a one-launch step beats the two-launch stream there (round 3,
    // in-process interleaved, profiles/ab_r03/band_r03u.err, band_r03w.err; µs per step,
    // two launches / one WG per env / flat step): N = 30 at 2,048 envs 27.2 / 24.7 / 25.9,
    // 3,072 36.3 / 34.7 / 36.3; N = 16 at 4,096 28.8 / 28.1 / 26.8, 6,144 38.1 / 39.8 / 36.9;
    // N = 8 at 4,096 19.4 / 18.9 / 16.3, 8,192 29.1 / 30.5 / 27.2; N = 32 at 3,072 37.9 /
    // 38.4 / 36.7; N = 64 at 1,024 28.6 / - / 26.8. From ~115 MiB the two-launch stream
    // leads (N = 30 at 4,096 44.8 / 45.7 / 47.2, N = 32 / 16 / 8 at 125 MiB, N = 48 at 188).
    // Which one-launch form: the one-WG-per-env step where its waves' chunk slots hold the
    // env with >= 90 % occupancy (N = 30: 1,875 of 2,048; it wins by 5-8 % there), else
    // the flat step (N = 8 / 16 / 32: 65 / 78 / 87 %, the flat step wins by 4-14 %) — the
    // same rule from 24 MiB, where the flat step also wins at N = 8 and 16 (4,096 x 8:
    // 16.3 vs 18.9 us; 3,072 x 16: 21.6 vs 22.6).
    if (win > (24ll << 20) && win <= (100ll << 20)) {
        const double one_fill = p.one_ok ? (double)p.per4 / (256.0 * p.one_waves) : 0.0;
        if (p.one_ok && one_fill >= 0.9) {
            p.one_auto |= PMENV_FUSE_INPLACE;
        } else if (p.flat1_ok && c.num_assets <= 64) {
            p.flat1_auto |= PMENV_FUSE_INPLACE;
            p.one_auto &= ~PMENV_FUSE_INPLACE;
        } else if (p.one_ok) {
            p.one_auto |= PMENV_FUSE_INPLACE;
        }
    }

    // ---- the relayed one-launch step (step_relay_kernel): the flat stream's shapes (F = 5,
    // W >= 2, 16-B granular env windows) with the two-launch path's scalar step forms
    // (N <= 512, the packed forms' [B*N] descriptors under 2^32 bytes), the stream's tile
    // geometry; at most BLOCK rows per tile (4 * 2 <= W * F).
    {
        const int N = c.num_assets;
        const int kv = p.k1_vec >= kK1Str ? p.k1_vec - kK1Str : p.k1_vec;
        p.relay_block = p.flat_ip_block;
        p.relay_v = 2;
        // a tile stages one row per thread: 4 CPW / (W F) + 2 rows must fit its BLOCK threads
        // (for V = 2: W >= 2; the host schedule emulation under tests/ checks it per tile)
        const bool rows_fit = 4 * p.relay_block * p.relay_v / (c.window * 5) + 2 <= p.relay_block;
        p.relay_ok = p.flat_ok && c.window >= 2 && rows_fit && N <= 512 && (N <= 64 || p.k1_vec != 0);
        p.relay_kl = kv ? kv / 100 : (N <= 32 ? 32 : 64);
        p.relay_ka = kv ? kv % 100 : 0;
        p.relay_auto = 0;
    }
    // AUTO gives the relay step the cache-resident windows where the kernel boundary of two
    // launches, or the scalar step inside every tile, is what a step pays for (N <= 64,
    // round 4, in-process interleaved, profiles/ab_r04/relay_band_r04b.err; us per step,
    // AUTO's previous choice / relay): in place 24-256 MiB — N = 30 at 2,048 / 3,072 / 4,096 /
    // 6,144 / 8,192 envs 24.9 / 23.7, 34.5 / 32.1, 44.3 / 40.6, 62.1 / 58.3, 81.9 / 80.0 (with
    // commission 83.6 / 80.6), N = 8 at 4,096 / 8,192 / 16,384 16.2 / 14.5, 27.7 / 24.3, 46.4 /
    // 42.7, N = 16 at 4,096 / 8,192 27.6 / 24.4, 46.4 / 42.4, N = 64 at 2,048 / 4,096 46.6 /
    // 43.1, 85.9 / 84.3 — except 24-48 MiB where the one-workgroup-per-env step holds the env
    // at >= 90 % (1,024 x 30: 13.5 / 14.9); double-buffered 48-128 MiB (2,048 / 4,096 x 30:
    // 27.2 / 23.2, 49.1 / 41.6; 8,192: 83.2 / 90.6). From 256 MiB in place the flat step leads
    // (12,288 / 16,384 / 65,536 x 30: 119.0 / 120.5, 156.8 / 159.9, 625.5 / 641.7), and at
    // config 5 two launches (1,324.6 / 1,360.3).
    if (p.relay_ok && c.num_assets <= 64) {
        const double one_fill = p.one_ok ? (double)p.per4 / (256.0 * p.one_waves) : 0.0;
        const bool one_holds = p.one_ok && one_fill >= 0.9 && win <= (48ll << 20);
        if (win > (24ll << 20) && win <= (256ll << 20) && !one_holds) p.relay_auto |= PMENV_FUSE_INPLACE;
        if (win > (48ll << 20) && win <= (128ll << 20)) p.relay_auto |= PMENV_FUSE_DB;
        p.one_auto &= ~p.relay_auto;
        p.flat1_auto &= ~p.relay_auto;
        // 256 x 4 tiles (16 KiB) for the largest cache-resident in-place windows, 192-256 MiB,
        // with the register-form scalar step of 17 <= N <= 32: config 4's 8-GPU share, 8,192 x
        // 30 in place, 78.6 vs 81.5 us (profiles/r06/relay_stamps/geom_8192x30.err; round 4: 76.8
        // vs 79.5 and 77.5 vs 78.1, ab_r04/relay_geom*); at 4,096 x 30 (123 MB) they lose
        // (42.3 vs 41.1), so 256 x 2 stays below
        const bool rows_fit4 = 4 * 256 * 4 / (c.window * 5) + 2 <= 256;
        if ((p.relay_auto & PMENV_FUSE_INPLACE) && win > (192ll << 20) && p.relay_block == 256 &&
            p.relay_kl == 32 && p.relay_ka == 0 && rows_fit4)
            p.relay_v = 4;
    }
    // ---- the generic stream (advance_gen_kernel, F != 5): 2 <= F <= 16 (its halo is the two
    // chunks past a workgroup, four past F = 8), 16-B granular env windows, at most BLOCK rows
    // per workgroup.
    // AUTO gives it every window above 2 MiB (16 MiB where step_tiny_kernel would take it),
    // both modes: against the register step / the LDS fallback, one process, the same bits
    // (profiles/ab_r05/gen_few_r05gf2.*), 64 / 256 x 30 x 50 x 8 in place 9.2 / 11.2 against
    // 12.8 / 14.2 us, 128 x 30 x 50 x 3 8.7 vs 9.2, 32 x 64 x 50 x 8 8.6 vs 16.4, 64 x 100 x 50 x 8
    // 10.9 vs 24.4 (LDS fallback), 2,048 x 128 x 50 x 4 double-buffered 76.8 vs 91.8; ties at 1-2
    // MiB (128 x 16 x 32 x 8 8.9 / 8.9, 64 x 16 x 32 x 8 9.0 vs 8.8); over tiny windows 1,024 x 5 x
    // 50 x 8 (8 MiB) 9.9 vs 7.8, 4,096 x 5 x 50 x 8 17.1 / 17.0, 4,096 x 8 x 32 x 6 14.9 vs 16.7
    {
        const int F = c.features;
        // 512 x 2 chunks per workgroup for windows past 128 MiB, 256 x 2 below (gen_geom_*_r05gg.*,
        // against 256 x 4: 65,536 x 30 x 50 x 8 in place / double-buffered 1,015.5 / 1,033.2 vs
        // 1,061.6 / 1,069.0 us, F = 3 / 4 388.8 / 514.9 vs 406.9 / 537.4, 16,384 x 30 x 50 x 8
        // 254.1 vs 268.3; within 2 % of 256 x 2 at 4,096 envs and below)
        p.gen_block = win > (128ll << 20) ? 512 : 256;
        p.gen_v = 2;
        const int64_t cpw = 1024;                           // the shape rule at the larger tile
        p.gen_ok = F != 5 && F >= 2 && F <= 16 && per % 4 == 0 &&
                   (int64_t)c.num_envs * (per / 4) < (1ll << 31) - 1024 && 4 * cpw / WF + 2 <= 256;
        p.gen_qtot = p.gen_ok ? (uint32_t)((int64_t)c.num_envs * (per / 4)) : 0u;
        p.gen_auto = p.gen_ok && win > (p.tiny ? (16ll << 20) : (2ll << 20)) ? (PMENV_FUSE_DB | PMENV_FUSE_INPLACE) : 0;
    }
    return PMENV_OK;
}

// What follows the tools build's plan hook (which may have rewritten geometry and AUTO's
// bits): the fields derived from them, the initial selection, the launch limits and the
// sizes of the handle's allocations.
inline int step_plan_finish(StepPlan* plan, const pmenv_cfg& c, char* err, size_t err_len) {
    using namespace pmenv_dev;
    StepPlan& p = *plan;
    if (p.streaming) {
        p.units_per_env = (c.num_assets + p.unit_rows - 1) / p.unit_rows;
        p.units_per_env_db = (c.num_assets + p.unit_rows_db - 1) / p.unit_rows_db;
    }
    p.path = PMENV_STEP_PATH_AUTO;
    p.one = p.one_auto;
    p.flat1 = p.flat1_auto;
    p.relay = p.relay_ok ? p.relay_auto : 0;
    p.gen = p.gen_ok ? p.gen_auto : 0;

    p.scalar_scratch_floats = (int)((scratch_bytes(0, c.num_assets, c.features) / 4 + 3) / 4 * 4);
    p.lds_scalar = (size_t)kScalarWaves * p.scalar_scratch_floats * 4;
    if (p.lds_tile > 160 * 1024 || p.lds_scalar > 160 * 1024)
        return plan_err(err, err_len, "num_assets %d needs more than 160 KiB of LDS", c.num_assets);
    if ((int64_t)c.num_envs * (p.streaming ? (p.units_per_env > p.units_per_env_db ? p.units_per_env
                                                                                  : p.units_per_env_db)
                                           : 1) >= (1ll << 31))
        return plan_err(err, err_len, "too many envs for one launch");

    const size_t B = (size_t)c.num_envs, BN = B * (size_t)c.num_assets;
    if (p.flat_inplace || p.gen_ok) {
        const uint32_t cpw = (uint32_t)(p.flat_inplace ? p.flat_ip_block * p.flat_ip_vec : p.gen_block * p.gen_v);
        const uint32_t qtot = p.flat_inplace ? p.flat_qtot : p.gen_qtot;
        const uint32_t wgs = (qtot + cpw - 1) / cpw;
        p.halo_wgs = wgs > 0 ? wgs - 1 : 0;
        const size_t per_wg = !p.flat_inplace && c.features > 8 ? 64 : 32;   // four chunks past F = 8
        p.halo_bytes = (size_t)(p.halo_wgs + 1) * per_wg;
    }
    if (p.flat1_ok) {
        // two parities of the snapshot (16-B aligned fields) and of the tile halo
        const uint32_t cpw = (uint32_t)(p.flat1_block * p.flat1_vec);
        const uint32_t wgs = (p.flat_qtot + cpw - 1) / cpw;
        p.halo1_wgs = wgs > 0 ? wgs - 1 : 0;
        p.snap_state_bytes = up16(B * 8) + up16(B * 4) + 2 * up16(BN * 4);
        p.snap_halo_bytes = up16(((size_t)p.halo1_wgs + 1) * 32);
        p.snap_bytes = 2 * (p.snap_state_bytes + p.snap_halo_bytes) + 64;
    }
    if (p.relay_ok) {
        const uint32_t cpw = (uint32_t)(p.relay_block * p.relay_v);
        p.relay_epb = (p.relay_block / 64) * (64 / p.relay_kl);
        p.relay_tiles = (p.flat_qtot + cpw - 1) / cpw;
        p.relay_scal = (uint32_t)(((uint64_t)c.num_envs + (uint64_t)p.relay_epb - 1) / (uint64_t)p.relay_epb);
        p.relay_words_bytes = up16(BN * 8) + relay_list_bytes(&p);
        p.relay_kp_bytes = up16(B * 4);
        p.relay_halo_bytes = up16((size_t)p.relay_tiles * 32);
        p.relay_bytes = 64 + p.relay_words_bytes + 2 * p.relay_kp_bytes + 2 * p.relay_halo_bytes;
    }
    return PMENV_OK;
}

// pmenv_set_step_path's rule: which windows (PMENV_FUSE_* bits) each step form takes under
// `path`. PMENV_ERR_ARG, the plan unchanged, for an unknown path or one the shape does not fit.
inline int step_plan_select(StepPlan* plan, int path) {
    const StepPlan& p = *plan;
    const int both = PMENV_FUSE_DB | PMENV_FUSE_INPLACE;
    int one = 0, flat1 = 0, relay = 0, gen = 0;
    switch (path) {
    case PMENV_STEP_PATH_AUTO:
        one = p.one_auto; flat1 = p.flat1_auto; relay = p.relay_auto; gen = p.gen_auto;
        break;
    case PMENV_STEP_PATH_ONE_LAUNCH:
        if (!p.one_ok) return PMENV_ERR_ARG;
        one = both;
        break;
    case PMENV_STEP_PATH_TWO_LAUNCH:
        if (!p.streaming && !p.gen_ok) return PMENV_ERR_ARG;
        gen = p.gen_ok ? both : 0;
        break;
    case PMENV_STEP_PATH_FLAT:
        if (!p.flat1_ok) return PMENV_ERR_ARG;
        flat1 = both;
        break;
    case PMENV_STEP_PATH_RELAY:
        if (!p.relay_ok) return PMENV_ERR_ARG;
        relay = both;
        break;
    default: return PMENV_ERR_ARG;
    }
    plan->path = path;
    plan->one = one;
    plan->flat1 = flat1;
    plan->relay = relay;
    plan->gen = gen;
    return PMENV_OK;
}

// What a step launches: pmenv_step_ex's precedence, written once.
enum StepRoute {
    kRouteFlat1,          // step_flat_kernel / step_flat_vec_kernel
    kRouteRelay,          // step_relay_kernel
    kRouteSurfaceStream,  // surface mode past the Infinity Cache: the scalar step, then surface_stream_kernel
    kRouteSurface,        // surface mode: step_surface_kernel
    kRouteOne,            // step_env_kernel
    kRouteTwoLaunch,      // the scalar step, then the F = 5 window stream
    kRouteGen,            // the scalar step, then advance_gen_kernel
    kRouteSmall,          // step_small_kernel / step_tiny_kernel
    kRouteLds             // step_advance_lds_kernel
};

// surface: the step has no bar. fuse_bit: PMENV_FUSE_INPLACE or PMENV_FUSE_DB, the window mode
// of an advance step. obs16: the windows the step touches are 16-B aligned (advance: obs and
// obs_out; surface: obs).
inline StepRoute step_route(const StepPlan& p, bool surface, int fuse_bit, bool obs16) {
    if (!surface && p.streaming && obs16 && (p.flat1 & fuse_bit)) return kRouteFlat1;
    if (!surface && p.streaming && obs16 && (p.relay & fuse_bit)) return kRouteRelay;
    if (surface) return p.surf_stream && obs16 ? kRouteSurfaceStream : kRouteSurface;
    if (p.streaming && obs16) return (p.one & fuse_bit) ? kRouteOne : kRouteTwoLaunch;
    if (p.gen_ok && (p.gen & fuse_bit) && obs16) return kRouteGen;
    return p.small_block ? kRouteSmall : kRouteLds;
}

enum {
    kDescribeFlatSeq = 1,    // the handle's flat steps are device-sequenced
    kDescribeRelaySeq = 2,   // the handle's relay steps are device-sequenced
    kDescribeDetail = 4      // append the geometry
};

// pmenv_step_path's string: per window mode (16-B aligned windows) the one-launch kernel, or
// the scalar step (K1) then the stream; one name where neither mode streams. With
// kDescribeDetail the plan's geometry follows as fixed key=value fields.
inline void step_plan_describe(const StepPlan& p, const pmenv_cfg& c, int flags, char* out, size_t size) {
    const char* k1 = p.k1_vec ? "scalar_step_vec_kernel"
                   : c.num_assets <= 64 ? "scalar_step_reg_kernel" : "scalar_step_kernel";
    char part[2][128];
    bool stream[2];
    for (int m = 0; m < 2; ++m) {          // 0 = double-buffered (obs_out), 1 = in place
        const StepRoute r = step_route(p, false, m ? PMENV_FUSE_INPLACE : PMENV_FUSE_DB, true);
        const char* name = "";
        const char* k2 = nullptr;
        switch (r) {
        case kRouteFlat1: name = c.num_assets > 64 ? "step_flat_vec_kernel" : "step_flat_kernel"; break;
        case kRouteRelay: name = "step_relay_kernel"; break;
        case kRouteOne: name = "step_env_kernel"; break;
        case kRouteTwoLaunch:
            k2 = m ? (p.flat_inplace ? "advance_flat_inplace_kernel" : "advance_rows_kernel")
                   : (p.flat ? "advance_flat_wg_kernel" : "advance_rows_kernel");
            break;
        case kRouteGen: k2 = "advance_gen_kernel"; break;
        case kRouteSmall: name = p.tiny ? "step_tiny_kernel" : "step_small_kernel"; break;
        default: name = "step_advance_lds_kernel"; break;
        }
        stream[m] = r != kRouteSmall && r != kRouteLds;
        if (k2) snprintf(part[m], sizeof part[m], "%s+%s", k1, k2);
        else snprintf(part[m], sizeof part[m], "%s", name);
    }
    int at;
    if (!stream[0] && !stream[1])
        at = snprintf(out, size, "%s", part[0]);
    else
        at = snprintf(out, size, "%s (obs_out) | %s (in place)%s%s", part[0], part[1],
                      (flags & kDescribeFlatSeq) && p.flat1 ? " [flat steps device-sequenced]" : "",
                      (flags & kDescribeRelaySeq) && p.relay ? " [relay steps device-sequenced]" : "");
    if (!(flags & kDescribeDetail) || at < 0 || (size_t)at >= size) return;
    char k1s[16];
    const int kv = p.k1_vec >= kK1Str ? p.k1_vec - kK1Str : p.k1_vec;
    if (kv) snprintf(k1s, sizeof k1s, "%dx%d%s", kv / 100, kv % 100, p.k1_vec >= kK1Str ? "s" : "");
    else snprintf(k1s, sizeof k1s, "%s", c.num_assets <= 64 ? "reg" : "lds");
    snprintf(out + at, size - (size_t)at,
             " -- flat1=%dx%d relay=%dx%d:%d/%d stream_ip=%dx%d pol=%d/%d gen=%dx%d k1=%s one_waves=%d small=%dx%d "
             "tiny=%d surf_stream=%d rows_per_tile=%d vec=%d",
             p.flat1_block, p.flat1_vec, p.relay_block, p.relay_v, p.relay_kl, p.relay_ka, p.flat_ip_block,
             p.flat_ip_vec, p.flat_pol, p.flat_ip_pol, p.gen_block, p.gen_v, k1s, p.one_waves, p.small_block,
             p.small_e, (int)p.tiny, (int)p.surf_stream, p.rows_per_tile, (int)p.vec);
}

// The whole of it for one cfg and path, as pmenv_step_path_for gives it: "" where
// pmenv_create refuses the cfg or pmenv_set_step_path the path.
inline void step_plan_path_for(const pmenv_cfg& c, int path, bool detail, char* out, size_t size) {
    StepPlan p;
    if (size) out[0] = 0;
    if (step_plan(c, &p, nullptr, 0) != PMENV_OK || step_plan_finish(&p, c, nullptr, 0) != PMENV_OK ||
        step_plan_select(&p, path) != PMENV_OK)
        return;
    step_plan_describe(p, c, detail ? kDescribeDetail : 0, out, size);
}

}  // namespace pmenv_host
