// pmenv.hip — host side and C ABI (include/pmenv.h) of the MI355X-native vectorised
// portfolio environment: the product library, libpmenv.so. Device code lives in
// step_flat.h (the one-launch step over fixed window tiles), step_env.h (the one-launch
// step, one workgroup per env), env_step.h (scalar step, window streams, reset,
// fallbacks), scalar_vec.h (packed scalar step), data.h (synthetic market data),
// rollout.h (GAE, moments), replay.h (replay gather, metrics), metrics_env.h (the metrics
// per episode) and trainer.h (batched reward); the step's launchers in launch.h, the
// handle in handle.h, features.h (fractional differencing, column scalers; their plan in
// ffd_plan.h), indicators.h (the technical indicators; their plan in ind_plan.h), adf.h (the
// search for the orders of differencing; its plan in adf_plan.h), its shape plan — which kernel a step takes, in which geometry — in
// step_plan.h, the sample gathers' kernel choice in replay_plan.h (both host only).
//
// Every entry point enqueues on the caller's stream and never synchronises, allocates or
// frees (graph-capturable), except create / destroy / the explicit synchronous queries
// documented in the header. Kernel choice is a function of the shape and of
// pmenv_set_step_path only: this library reads no environment variable. The A/B
// alternatives measured while choosing live in the tools build (tools/ab/pmenv_ab.hip,
// linked with this file into tools/libpmenv_ab.so), behind the pmenv_tools hooks whose
// definitions here, at the end of the file, do nothing.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <type_traits>

#include "../../include/pmenv.h"
#include "adf.h"
#include "adf_plan.h"
#include "data.h"
#include "episode.h"
#include "features.h"
#include "ffd_plan.h"
#include "handle.h"
#include "ind_plan.h"
#include "indicators.h"
#include "launch.h"
#include "metrics_env.h"
#include "prio.h"
#include "replay.h"
#include "replay_valid.h"
#include "replay_plan.h"
#include "rollout.h"
#include "step_plan.h"
#include "trainer.h"

using namespace pmenv_dev;
using namespace pmenv_host;

namespace {

thread_local char g_create_err[512] = "";

// calls f(std::integral_constant<int, V>()) for the V among Vs that equals v: a planned
// pairs-per-thread or store-policy value becomes a kernel's template argument
template <int... Vs, class Fn>
void with_const(int v, Fn&& f) {
    (void)((v == Vs && (f(std::integral_constant<int, Vs>()), true)) || ...);
}
// replay_plan's `aligned` bits: every window output, and the series, 16-B aligned
int replay_aligned(const void* out0, const void* out1, const void* series) {
    return ((((uintptr_t)out0 | (uintptr_t)out1) & 15u) == 0 ? kReplayOutAligned : 0) |
           (((uintptr_t)series & 15u) == 0 ? kReplaySeriesAligned : 0);
}

// the stream is being captured into a hipGraph: step_flat_kernel's host-chosen parity
// would be frozen under replay, so the handle switches to the device-sequenced form
bool capturing(hipStream_t stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    return st != hipStreamCaptureStatusNone;
}

// Anything but step_flat_kernel that writes the state or a window leaves the snapshot and
// the halo stale (`what` = the device words to clear: V, the snapshot-valid word, or HOBS,
// the window the halo belongs to). The host flags cover eager steps; device-sequenced
// handles also clear the device word on the stream. An invalidation enqueued while the
// stream is being captured switches the handle to the device-sequenced form first: a
// graph of [reset, flat steps] replays the reset's clear before every replay's steps,
// where host flags set once at capture time would let replay 2 on read the snapshot the
// previous replay left (flat_seq_kernel then re-primes from the reset state).
enum { kInvalSnap = 1, kInvalHalo = 2 };
// Once any call of this handle is enqueued while `stream` is being captured into a hipGraph,
// replays may write the window or the state where the host does not see it: from then on the
// flat and the relay steps keep the validity of their copies (snapshot, counter copy, halo) in
// device words that every invalidation clears on the stream — whatever path is current when the
// capture is seen, since a later switch of path must not find host flags a replay outdated.
void note_capture(pmenv* h, hipStream_t stream) {
    if (((h->flat1_ok && !h->device_seq) || (h->relay_ok && !h->relay_dseq)) && capturing(stream)) {
        if (h->flat1_ok) h->device_seq = true;
        if (h->relay_ok) h->relay_dseq = true;
    }
}

// the relay step's copies go stale (kInvalSnap: the counter copy and the halo; kInvalHalo: the halo)
int relay_invalidate(pmenv* h, hipStream_t stream, int what) {
    h->relay_obs = nullptr;
    if (what & kInvalSnap) h->relay_kp_ok = false;
    if (!h->relay_dseq || !h->relay_mem) return PMENV_OK;
    // V = 0 re-primes both, HOBS = 0 the halo
    const hipError_t e = (what & kInvalSnap) ? hipMemsetAsync(h->relay_seq + 2, 0, 4, stream)
                                             : hipMemsetAsync(h->relay_seq + 6, 0, 8, stream);
    if (e != hipSuccess) {
        set_err(h, "invalidating the relay step's copies: %s", hipGetErrorString(e));
        return PMENV_ERR_HIP;
    }
    return PMENV_OK;
}

int flat1_invalidate(pmenv* h, hipStream_t stream, int what = kInvalSnap | kInvalHalo, bool host_only = false,
                     bool keep_relay = false) {
    if (what & kInvalSnap) h->snap_ok = false;
    h->halo1_obs = nullptr;
    if (!host_only) note_capture(h, stream);
    if (!keep_relay) {
        if (host_only) {
            h->relay_obs = nullptr;
            if (what & kInvalSnap) h->relay_kp_ok = false;
        } else if (const int rc = relay_invalidate(h, stream, what)) {
            return rc;
        }
    }
    if (host_only || !h->device_seq) return PMENV_OK;
    // V = 0 clears both (a stale V re-primes the halo too); HOBS = 0 only the halo
    const hipError_t e = (what & kInvalSnap) ? hipMemsetAsync(h->seq + 2, 0, 4, stream)
                                             : hipMemsetAsync(h->seq + 4, 0, 8, stream);
    if (e != hipSuccess) {
        set_err(h, "invalidating the flat step's snapshot: %s", hipGetErrorString(e));
        return PMENV_ERR_HIP;
    }
    return PMENV_OK;
}

// The relay step's memory (zeroed: the device-sequenced words, no relay word, deferral list or tile
// claim of any epoch), allocated when AUTO gives the shape the relay step or pmenv_set_step_path asks
// for it — not on a step. The deferral list and claims (step_relay.h) follow the relay words, so
// one memset clears all three when the eager epoch wraps.
int relay_alloc(pmenv* h) {
    if (h->relay_mem || !h->relay_ok) return PMENV_OK;
    const size_t BN = (size_t)h->cfg.num_envs * (size_t)h->cfg.num_assets;
    const size_t ctl_b = 64, words_b = h->relay_words_bytes, kp_b = h->relay_kp_bytes, hal = h->relay_halo_bytes;
    const size_t bytes = h->relay_bytes;
    DeviceGuard g(h->device);
    void* m = nullptr;
    hipError_t ae = hipMalloc(&m, bytes);
    if (ae != hipSuccess) {
        set_err(h, "hipMalloc(relay) failed: %s", hipGetErrorString(ae));
        return PMENV_ERR_HIP;
    }
    ae = hipMemset(m, 0, ctl_b + words_b);
    if (ae != hipSuccess) {
        (void)hipFree(m);
        set_err(h, "relay words: %s", hipGetErrorString(ae));
        return PMENV_ERR_HIP;
    }
    char* b = (char*)m;
    h->relay_mem = m;
    h->relay_seq = (uint32_t*)b;
    h->relay_w = (uint64_t*)(b + ctl_b);
    h->relay_list = (uint64_t*)(b + ctl_b + up16(BN * 8));
    h->relay_done = (uint32_t*)(b + ctl_b + up16(BN * 8) + up16(((size_t)h->relay_tiles + 1) * 8));
    h->relay_kp = (int32_t*)(b + ctl_b + words_b);
    h->relay_halo = (float*)(b + ctl_b + words_b + 2 * kp_b);
    h->relay_halo_stride = (uint32_t)(hal / 4);
    h->relay_obs = nullptr;
    h->relay_kp_ok = false;
    h->relay_par = 0;
    h->relay_epoch = 0;
    return PMENV_OK;
}

}  // namespace

extern "C" {

int32_t pmenv_abi_version(void) { return PMENV_ABI_VERSION; }

void pmenv_cfg_default(pmenv_cfg* cfg, int32_t num_envs, int32_t num_assets, int32_t window, int32_t features) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->num_envs = num_envs;
    cfg->num_assets = num_assets;
    cfg->window = window;
    cfg->features = features;
    cfg->close_channel = features >= 5 ? 3 : 0;
    cfg->reward_kind = PMENV_REWARD_LOG_RETURN;
    cfg->norm_mode = PMENV_NORM_AND;
    cfg->ring_mode = PMENV_RING_STORAGE;
    cfg->ret_mode = PMENV_RET_GROSS;
    cfg->mu_max_iter = 100;
    cfg->init_cash = 25000.0;
    cfg->commission = 0.0;
    cfg->reward_scale = 1.0;
    cfg->risk_free_rate = 0.04;
    cfg->sharpe_eta = 0.01;
    cfg->mu_tol = 1e-10;
}

const char* pmenv_last_error(const pmenv* h) { return h ? h->err : g_create_err; }

int pmenv_get_cfg(const pmenv* h, pmenv_cfg* out) {
    if (!h || !out) return PMENV_ERR_ARG;
    *out = h->cfg;
    return PMENV_OK;
}

int pmenv_state_layout(const pmenv_cfg* cfg, size_t off[PMENV_STATE_FIELDS]) {
    if (!cfg || !off || cfg->num_envs < 1 || cfg->num_assets < 1 || cfg->window < 1) return PMENV_ERR_ARG;
    const size_t B = (size_t)cfg->num_envs, N = (size_t)cfg->num_assets;
    const size_t ring_elems = B * (size_t)cfg->window * N;
    auto up16 = [](size_t x) { return (x + 15) / 16 * 16; };
    size_t o = 0;
    off[0] = o; o = up16(o + B * 8);           // value
    off[1] = o; o = up16(o + B * 8);           // stat_a
    off[2] = o; o = up16(o + B * 8);           // stat_b
    off[3] = o; o = up16(o + B * 4);           // counter
    off[4] = o; o = up16(o + ring_elems * 4);  // ring
    off[5] = o; o = up16(o + 8);               // nonfinite
    off[6] = o; o = up16(o + B * N * 4);       // last_close
    off[7] = o;                                // w_new
    return PMENV_OK;
}

size_t pmenv_state_bytes_for(const pmenv_cfg* cfg) {
    size_t off[PMENV_STATE_FIELDS];
    if (pmenv_state_layout(cfg, off) != PMENV_OK) return 0;
    return (off[7] + (size_t)cfg->num_envs * cfg->num_assets * 4 + 15) / 16 * 16;
}

int pmenv_create(const pmenv_cfg* cfg, int device, pmenv** out) {
    return pmenv_create_in(cfg, device, nullptr, 0, out);
}

int pmenv_create_in(const pmenv_cfg* cfg, int device, void* state, size_t state_bytes, pmenv** out) {
    if (!cfg || !out) return PMENV_ERR_ARG;
    *out = nullptr;
    pmenv* h = (pmenv*)calloc(1, sizeof(pmenv));
    if (!h) return PMENV_ERR_ARG;
    h->cfg = *cfg;
    h->device = device;
    const pmenv_cfg& c = h->cfg;
    auto fail = [&](int code) {
        // no handle reaches the caller: pmenv_last_error(NULL) reports this one
        snprintf(g_create_err, sizeof(g_create_err), "%s", h->err);
        pmenv_tools::release(h);
        if (h->state && h->owns_state) (void)hipFree(h->state);
        if (h->halo) (void)hipFree(h->halo);
        if (h->snap) (void)hipFree(h->snap);
        if (h->relay_mem) (void)hipFree(h->relay_mem);
        free(h);
        return code;
    };
    // the shape plan (step_plan.h): the argument checks and every kernel choice; the tools
    // build's PMENV_* knobs rewrite it before the sizes that follow from it are taken
    if (const int rc = step_plan(c, h, h->err, sizeof(h->err))) return fail(rc);
    if (h->cfg.ret_mode == PMENV_RET_AUTO)
        h->cfg.ret_mode = c.reward_kind == PMENV_REWARD_LOG_RETURN ? PMENV_RET_GROSS : PMENV_RET_NET;
    pmenv_tools::plan(h);     // nothing in the product library
    if (const int rc = step_plan_finish(h, c, h->err, sizeof(h->err))) return fail(rc);

    DeviceGuard g(device);
    size_t off[PMENV_STATE_FIELDS];
    pmenv_state_layout(&c, off);
    h->state_bytes = pmenv_state_bytes_for(&c);
    if (state) {
        if (state_bytes < h->state_bytes || ((uintptr_t)state & 15u)) {
            set_err(h, "caller state buffer too small (%zu < %zu) or not 16-B aligned", state_bytes, h->state_bytes);
            return fail(PMENV_ERR_ARG);
        }
        h->state = state;
        h->owns_state = false;
    } else {
        hipError_t ae = hipMalloc(&h->state, h->state_bytes);
        if (ae != hipSuccess) {
            set_err(h, "hipMalloc(%zu) failed: %s", h->state_bytes, hipGetErrorString(ae));
            h->state = nullptr;
            return fail(PMENV_ERR_HIP);
        }
        h->owns_state = true;
    }
    if (h->halo_bytes) {
        hipError_t ae = hipMalloc(&h->halo, h->halo_bytes);
        if (ae != hipSuccess) {
            set_err(h, "hipMalloc(halo) failed: %s", hipGetErrorString(ae));
            h->halo = nullptr;
            return fail(PMENV_ERR_HIP);
        }
    }
    if (h->flat1_ok) {
        // two parities of the snapshot (16-B aligned fields) and of the tile halo
        const size_t B = (size_t)c.num_envs, BN = B * (size_t)c.num_assets;
        const size_t one = h->snap_state_bytes, hal = h->snap_halo_bytes;
        hipError_t ae = hipMalloc(&h->snap, h->snap_bytes);
        if (ae != hipSuccess) {
            set_err(h, "hipMalloc(snapshot) failed: %s", hipGetErrorString(ae));
            h->snap = nullptr;
            return fail(PMENV_ERR_HIP);
        }
        for (int q = 0; q < 2; ++q) {
            char* sb = (char*)h->snap + (size_t)q * (one + hal);
            h->sv[q] = (double*)sb;
            h->sk[q] = (int32_t*)(sb + up16(B * 8));
            h->sw[q] = (float*)(sb + up16(B * 8) + up16(B * 4));
            h->slc[q] = (float*)(sb + up16(B * 8) + up16(B * 4) + up16(BN * 4));
            h->halo1[q] = (float*)(sb + one);
        }
        h->snap_stride = one + hal;
        h->seq = (int32_t*)((char*)h->snap + 2 * (one + hal));
        if (hipMemset(h->seq, 0, 64) != hipSuccess) {
            set_err(h, "hipMemset(seq) failed");
            return fail(PMENV_ERR_HIP);
        }
    }
    if (h->relay && relay_alloc(h) != PMENV_OK) return fail(PMENV_ERR_HIP);
    (void)flat1_invalidate(h, nullptr, kInvalSnap | kInvalHalo, true);   // no device sequencing yet
    char* base = (char*)h->state;
    h->value = (double*)(base + off[0]);
    h->sa = (double*)(base + off[1]);
    h->sb = (double*)(base + off[2]);
    h->k = (int32_t*)(base + off[3]);
    h->ring = (float*)(base + off[4]);
    h->nonfinite = (unsigned long long*)(base + off[5]);
    h->last_close = (float*)(base + off[6]);
    h->w_new = (float*)(base + off[7]);
    const struct { const void* fn; size_t lds; } attrs[] = {
        {(const void*)step_advance_lds_kernel<true>, h->lds_tile},
        {(const void*)step_advance_lds_kernel<false>, h->lds_tile},
        {(const void*)step_surface_kernel, h->lds_surface},
        {(const void*)step_surface_host_kernel, h->lds_surface},
        {(const void*)step_host_resident_kernel, h->lds_surface},
        {(const void*)step_small_kernel<64, 32, false>, h->lds_surface},
        {(const void*)step_small_kernel<256, 8, false>, h->lds_surface},
        {(const void*)step_small_kernel<256, 16, false>, h->lds_surface},
        {(const void*)step_small_kernel<512, 16, false>, h->lds_surface},
        {(const void*)step_small_kernel<1024, 16, false>, h->lds_surface},
        {(const void*)scalar_step_kernel, h->lds_scalar},
    };
    for (const auto& a : attrs)   // only needed above 64 KiB; failures surface at launch
        if (hipFuncSetAttribute(a.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds) != hipSuccess)
            (void)hipGetLastError();
    hipError_t e = hipMemset(h->state, 0, h->state_bytes);
    if (e != hipSuccess) {
        set_err(h, "hipMemset failed: %s", hipGetErrorString(e));
        return fail(PMENV_ERR_HIP);
    }
    StepParams p = base_params(h);
    reset_kernel<<<c.num_envs, kBlock, 0, nullptr>>>(p, nullptr, nullptr);
    e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        set_err(h, "initial reset failed: %s", hipGetErrorString(e));
        return fail(PMENV_ERR_HIP);
    }
    *out = h;
    return PMENV_OK;
}

namespace {
void res_stop(pmenv* h);    // the resident host-I/O step (below)
}

int pmenv_destroy(pmenv* h) {
    if (!h) return PMENV_ERR_ARG;
    DeviceGuard g(h->device);
    pmenv_tools::release(h);
    if (h->state && h->owns_state) (void)hipFree(h->state);
    if (h->halo) (void)hipFree(h->halo);
    if (h->snap) (void)hipFree(h->snap);
    if (h->relay_mem) (void)hipFree(h->relay_mem);
    if (h->hio) {
        res_stop(h);
        (void)hipHostFree(h->hio);
    }
    if (h->res_stream) {
        (void)hipEventDestroy(h->res_ev);
        (void)hipStreamDestroy(h->res_stream);
        (void)hipFree(h->res_last);
    }
    free(h);
    return PMENV_OK;
}

int pmenv_set_step_path(pmenv* h, int32_t path) {
    if (!h) return PMENV_ERR_ARG;
    if (path < PMENV_STEP_PATH_AUTO || path > PMENV_STEP_PATH_RELAY) {
        set_err(h, "unknown step path %d", path);
        return PMENV_ERR_ARG;
    }
    StepPlan sel = *h;                     // the handle stays unchanged unless everything succeeds
    if (step_plan_select(&sel, path) != PMENV_OK) {
        set_err(h, "step path %d does not fit this shape (one launch: F = 5, W >= 2, N <= 64, window <= 64 KiB "
                   "of LDS; two launches: F = 5, 16-B granular env windows; flat: F = 5, W >= 2, N <= 64, "
                   "16-B granular env windows of >= 148 chunks, N > 64 up to 512 with W >= 14; relay: F = 5, "
                   "W >= 2, 16-B granular env windows, N <= 512)", path);
        return PMENV_ERR_ARG;
    }
    if (sel.relay && relay_alloc(h) != PMENV_OK) return PMENV_ERR_HIP;
    static_cast<StepPlan&>(*h) = sel;
    return PMENV_OK;
}

int pmenv_reset(pmenv* h, float* obs, const uint8_t* mask, hipStream_t stream) {
    if (!h) return PMENV_ERR_ARG;
    h->dev_pending = true;                          // device work of this handle may be in flight
    if (obs && !aligned4(obs)) { set_err(h, "obs not 4-byte aligned"); return PMENV_ERR_ALIGN; }
    DeviceGuard g(h->device);
    StepParams p = base_params(h);
    if (const int rc = flat1_invalidate(h, stream)) return rc;
    reset_kernel<<<h->cfg.num_envs, kBlock, 0, stream>>>(p, obs, mask);
    return check_launch(h, "reset_kernel");
}

int pmenv_restart_days(pmenv* h, float* obs, const float* series, int32_t series_days, int32_t* day,
                       const int32_t* end, const int32_t* restart, uint8_t* done, hipStream_t stream) {
    if (!h) return PMENV_ERR_ARG;
    h->dev_pending = true;                          // device work of this handle may be in flight
    const void* ptrs[6] = {obs, series, day, end, restart, done};
    static const char* const names[6] = {"obs", "series", "day", "end", "restart", "done"};
    for (int i = 0; i < 6; ++i) {
        if (!ptrs[i]) { set_err(h, "pmenv_restart_days: %s is required", names[i]); return PMENV_ERR_ARG; }
        if (i < 5 && !aligned4(ptrs[i])) {          // done is bytes
            set_err(h, "pmenv_restart_days: %s not 4-byte aligned", names[i]);
            return PMENV_ERR_ALIGN;
        }
    }
    if (series_days < 1) { set_err(h, "pmenv_restart_days: series_days must be >= 1"); return PMENV_ERR_ARG; }
    DeviceGuard g(h->device);
    StepParams p = base_params(h);
    // unconditional: with staggered envs some env restarts on nearly every call
    if (const int rc = flat1_invalidate(h, stream)) return rc;
    const pmenv_cfg& c = h->cfg;
    const unsigned grid = (unsigned)((c.num_envs + kEpSlice - 1) / kEpSlice);
    const size_t slab = (size_t)c.window * c.num_assets * 16;
    const bool staged = c.features == 5 && ((int64_t)c.num_assets * c.window * 5) % 4 == 0 &&
                        (((uintptr_t)obs | (uintptr_t)series | (uintptr_t)h->ring) & 15u) == 0 &&
                        kEpMaskBytes + slab <= kEpLdsMax;
    const auto kernel = staged ? restart_days_kernel<true> : restart_days_kernel<false>;
    kernel<<<grid, kEpBlock, kEpMaskBytes + (staged ? slab : 0), stream>>>(p, obs, series, series_days, day, end,
                                                                          restart, done);
    return check_launch(h, "restart_days_kernel");
}

int pmenv_step_ex(pmenv* h, const pmenv_step_args* a, hipStream_t stream) {
    if (!h) return PMENV_ERR_ARG;
    h->dev_pending = true;                          // device work of this handle may be in flight
    if (!a || !a->action) { set_err(h, "action is required"); return PMENV_ERR_ARG; }
    if (!a->bar && !a->prices) { set_err(h, "surface mode (bar == NULL) needs prices"); return PMENV_ERR_ARG; }
    if (a->bar && !a->obs) { set_err(h, "advance mode (bar != NULL) needs obs"); return PMENV_ERR_ARG; }
    if (!aligned4(a->action) || (a->prices && !aligned4(a->prices)) || (a->bar && !aligned4(a->bar)) ||
        (a->obs && !aligned4(a->obs)) || (a->reward && !aligned4(a->reward)) ||
        (a->weights && !aligned4(a->weights)) || (a->ret && ((uintptr_t)a->ret & 7u))) {
        set_err(h, "unaligned pointer");
        return PMENV_ERR_ALIGN;
    }
    DeviceGuard g(h->device);
    StepParams p = base_params(h);
    if (a->day && (!a->bar || a->series_days < 1)) {
        set_err(h, "day[] needs the series in bar and series_days >= 1");
        return PMENV_ERR_ARG;
    }
    p.action = a->action; p.prices = a->prices; p.bar = a->bar; p.obs = a->obs;
    p.day = a->day; p.series_days = a->series_days;
    p.obs_out = a->obs_out ? a->obs_out : a->obs;
    if (a->obs_out && a->bar) {
        const size_t bytes = (size_t)h->cfg.num_envs * h->cfg.num_assets * h->cfg.window * h->cfg.features * 4;
        const char *o0 = (const char*)a->obs, *o1 = (const char*)a->obs_out;
        if (!aligned4(a->obs_out) || (o1 < o0 + bytes && o0 < o1 + bytes)) {
            set_err(h, "obs_out must be 4-byte aligned and must not overlap obs");
            return PMENV_ERR_ARG;
        }
    }
    p.reward = a->reward; p.ret = a->ret; p.weights = a->weights;
    const int B = h->cfg.num_envs;
    const bool obs16 = (((uintptr_t)a->obs | (uintptr_t)p.obs_out) & 15u) == 0;
    const int fuse_bit = p.obs_out == p.obs ? PMENV_FUSE_INPLACE : PMENV_FUSE_DB;
    // surface steps touch obs alone
    const bool win16 = a->bar ? obs16 : (((uintptr_t)a->obs) & 15u) == 0;
    const uint32_t ph = a->phases ? a->phases : (PMENV_PHASE_SCALAR | PMENV_PHASE_ADVANCE);
    const StepRoute route = step_route(*h, !a->bar, fuse_bit, win16);
    if (route != kRouteFlat1 && route != kRouteRelay)
        if (const int rc = flat1_invalidate(h, stream)) return rc;   // every other path skips the snapshot
    switch (route) {
    case kRouteFlat1:
        // one launch over the flat stream: the whole step runs in the scalar phase
        if (!(ph & PMENV_PHASE_SCALAR)) return PMENV_OK;
        // a step captured into a hipGraph replays with frozen arguments: from then on this
        // handle sequences its flat steps on the device (flat_seq_kernel + the kernel)
        if (!h->device_seq && capturing(stream)) h->device_seq = true;
        note_capture(h, stream);
        // the relay step's halo and counter copy go stale
        if (const int rc = relay_invalidate(h, stream, kInvalSnap | kInvalHalo)) return rc;
        launch_flat1(h, p, stream);
        return check_launch(h, "step_flat_kernel");
    case kRouteRelay:
        // one launch, the scalar work relaying to the stream tiles (captured: device-sequenced)
        if (!(ph & PMENV_PHASE_SCALAR)) return PMENV_OK;
        if (const int rc = flat1_invalidate(h, stream, kInvalSnap | kInvalHalo, false, true)) return rc;
        if (launch_relay(h, p, stream) != PMENV_OK) {
            set_err(h, "relay step: hipMemsetAsync failed");
            return PMENV_ERR_HIP;
        }
        return check_launch(h, "step_relay_kernel");
    case kRouteSurfaceStream:
        // past the Infinity Cache: the scalar step, then the surface stream
        if (ph & PMENV_PHASE_SCALAR) {
            launch_scalar_kernels(h, p, stream);
            if (const int rc = check_launch(h, "scalar_step_kernel")) return rc;
        }
        if (ph & PMENV_PHASE_ADVANCE) {
            launch_surface_stream(h, p, stream);
            return check_launch(h, "surface_stream_kernel");
        }
        return PMENV_OK;
    case kRouteSurface:
        if (a->phases == PMENV_PHASE_ADVANCE) return PMENV_OK;   // single launch: done in the scalar phase
        step_surface_kernel<<<B, kBlock, h->lds_surface, stream>>>(p);
        return check_launch(h, "step_surface_kernel");
    case kRouteOne:                    // one launch: the whole step runs in the scalar phase
        if (!(ph & PMENV_PHASE_SCALAR)) return PMENV_OK;
        launch_one(h, p, stream);
        return check_launch(h, "step_env_kernel");
    case kRouteTwoLaunch:
        if (pmenv_tools::launch_fused(h, p, fuse_bit, ph, stream)) return check_launch(h, "tools: fused step");
        if (ph & PMENV_PHASE_SCALAR) {
            launch_scalar(h, p, stream);
            const int rc = check_launch(h, "scalar_step_kernel");
            if (rc) return rc;
        }
        if (ph & PMENV_PHASE_ADVANCE) {
            launch_advance(h, p, stream);
            return check_launch(h, "advance kernel");
        }
        return PMENV_OK;
    case kRouteGen:
        // F != 5: the scalar step (copying the in-place stream's halo), then the generic stream
        if (ph & PMENV_PHASE_SCALAR) {
            launch_scalar(h, p, stream);
            const int rc = check_launch(h, "scalar_step_kernel");
            if (rc) return rc;
        }
        if (ph & PMENV_PHASE_ADVANCE) {
            launch_gen(h, p, stream);
            return check_launch(h, "advance_gen_kernel");
        }
        return PMENV_OK;
    case kRouteSmall:
        if (a->phases == PMENV_PHASE_ADVANCE) return PMENV_OK;   // single-launch path: all done in the scalar phase
        launch_small(h, p, stream);
        return check_launch(h, h->tiny ? "step_tiny_kernel" : "step_small_kernel");
    case kRouteLds:
        break;
    }
    if (a->phases == PMENV_PHASE_ADVANCE) return PMENV_OK;       // single-launch path, likewise
    if (h->vec && obs16)
        step_advance_lds_kernel<true><<<B, kBlock, h->lds_tile, stream>>>(p);
    else
        step_advance_lds_kernel<false><<<B, kBlock, h->lds_tile, stream>>>(p);
    return check_launch(h, "step_advance_lds_kernel");
}

int pmenv_step(pmenv* h, const float* action, const float* prices, const float* bar, float* obs, float* reward,
               hipStream_t stream) {
    pmenv_step_args a;
    memset(&a, 0, sizeof(a));
    a.action = action; a.prices = prices; a.bar = bar; a.obs = obs; a.reward = reward;
    return pmenv_step_ex(h, &a, stream);
}

}  // extern "C"

namespace {
// The host-I/O staging block (allocated on first use, freed by destroy): f32 action |
// prices | closes [B*N] each, channel [B*N*W], weights [B*N], reward [B]; f64 return |
// value [B]; u32 completion words [B]; the resident step's go word. Pinned and device-mapped,
// so the kernels read and write it over PCIe directly.
int hio_ensure(pmenv* h) {
    if (h->hio) return PMENV_OK;
    const size_t B = (size_t)h->cfg.num_envs, BN = B * (size_t)h->cfg.num_assets;
    auto up64 = [](size_t x) { return (x + 63) / 64 * 64; };
    size_t o = 0;
    const size_t sizes[10] = {BN * 4, BN * 4, BN * 4, BN * (size_t)h->cfg.window * 4, BN * 4, B * 4, B * 8, B * 8,
                              B * 4, 4};
    for (int i = 0; i < 10; ++i) {
        h->hio_off[i] = o;
        o = up64(o + sizes[i]);
    }
    void* p = nullptr;
    // coherent (fine-grained): the GPU never caches it, so each step reads what the host
    // just wrote and the host reads the kernel's stores after the stream sync
    hipError_t e = hipHostMalloc(&p, o, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) {
        set_err(h, "hipHostMalloc(%zu) for host-I/O staging failed: %s", o, hipGetErrorString(e));
        return PMENV_ERR_HIP;
    }
    void* d = nullptr;
    e = hipHostGetDevicePointer(&d, p, 0);
    if (e != hipSuccess) {
        (void)hipHostFree(p);
        set_err(h, "hipHostGetDevicePointer: %s", hipGetErrorString(e));
        return PMENV_ERR_HIP;
    }
    h->hio = (char*)p;
    h->hio_dev = (char*)d;
    memset(h->hio + h->hio_off[8], 0, B * 4);      // completion words: no call yet (tags start at 1)
    memset(h->hio + h->hio_off[9], 0, 4);          // the go word: no tag posted
    h->hio_seq = 0;
    return PMENV_OK;
}
enum { kHioAct, kHioPri, kHioClose, kHioChan, kHioW, kHioRew, kHioRet, kHioVal, kHioDone, kHioGo };
template <class T>
T* hio_host(const pmenv* h, int f) { return reinterpret_cast<T*>(h->hio + h->hio_off[f]); }
template <class T>
T* hio_dev(const pmenv* h, int f) { return reinterpret_cast<T*>(h->hio_dev + h->hio_off[f]); }

// the window's last closes obs[b, n, W-1, close] -> staging (the only window bytes the step reads)
void hio_gather_closes(pmenv* h, const float* obs) {
    const pmenv_cfg& c = h->cfg;
    const size_t BN = (size_t)c.num_envs * c.num_assets, row = (size_t)c.window * c.features;
    const float* src = obs + (size_t)(c.window - 1) * c.features + c.close_channel;
    float* dst = hio_host<float>(h, kHioClose);
    for (size_t i = 0; i < BN; ++i) dst[i] = src[i * row];
}
// the [B, N, W] channel the kernel wrote -> obs[..., F-1] of the caller's window
void hio_scatter_channel(const pmenv* h, float* obs) {
    const pmenv_cfg& c = h->cfg;
    const size_t BNW = (size_t)c.num_envs * c.num_assets * c.window;
    const int F = c.features;
    const float* src = hio_host<float>(h, kHioChan);
    float* dst = obs + (F - 1);
    for (size_t i = 0; i < BNW; ++i) dst[i * F] = src[i];
}
// The call's completion: every env's completion word carries the call's tag once its outputs
// are in host memory (the kernels write it last, at system scope, after every store of the
// workgroup has completed). The host spins on the words — they turn a few us after the
// launch — instead of synchronising the stream: 12.3 / 14.8 us per pmenv_step_host call
// against 18.2 / 20.1 with hipStreamSynchronize at 1 x 5 x 50 x 5 / 1 x 32 x 32 x 5
// (profiles/hostio_r05/hostio_r05h*.json). Past ~2 ms (a large batch, or a kernel that
// failed) it synchronises the stream, which also reports an error.
int hio_sync(pmenv* h, hipStream_t stream, const char* what) {
    if (const int rc = check_launch(h, what)) return rc;
    const volatile uint32_t* done = hio_host<volatile uint32_t>(h, kHioDone);
    const uint32_t seq = h->hio_seq;
    const int B = h->cfg.num_envs;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t it = 0;; ++it) {
        int b = 0;
        while (b < B && done[b] == seq) ++b;
        if (b == B) {
            __atomic_thread_fence(__ATOMIC_ACQUIRE);        // the outputs are read after the words
            return PMENV_OK;
        }
        if ((it & 255u) == 255u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        set_err(h, "%s: %s", what, hipGetErrorString(e));
        return PMENV_ERR_HIP;
    }
    return PMENV_OK;
}

// ---- the resident host-I/O step (step_host_resident_kernel): no launch per call
constexpr int kResMaxEnvs = 8;             // one workgroup steps every env in turn
constexpr uint32_t kResIdle = 2000000u;    // 20 ms of s_memrealtime (100 MHz) without a call: it exits

// the workgroup exits (the stop tag) and the handle forgets it (destroy, or its launch
// arguments no longer match the call's)
void res_stop(pmenv* h) {
    if (!h->res_live) return;
    __atomic_store_n(hio_host<uint32_t>(h, kHioGo), 0u, __ATOMIC_RELEASE);
    (void)hipEventSynchronize(h->res_ev);
    h->res_live = false;
}

int res_launch(pmenv* h, const StepParams& p, const HostIO& io) {
    if (!h->res_stream) {
        if (hipStreamCreateWithFlags(&h->res_stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&h->res_ev, hipEventDisableTiming) != hipSuccess ||
            hipMalloc((void**)&h->res_last, 64) != hipSuccess || hipMemset(h->res_last, 0, 64) != hipSuccess) {
            set_err(h, "resident host-I/O step: stream / event / memory");
            return PMENV_ERR_HIP;
        }
    }
    // the go word holds the last tag posted (or 0): a fresh workgroup starts from what the
    // previous one ran, so an unseen tag is run and a seen one is not run twice
    HostRes rs;
    rs.go = hio_dev<uint32_t>(h, kHioGo);
    rs.last = h->res_last;
    rs.idle = kResIdle;
    step_host_resident_kernel<<<1, kBlock, h->lds_surface, h->res_stream>>>(p, io, rs);
    if (const int rc = check_launch(h, "step_host_resident_kernel")) return rc;
    if (hipEventRecord(h->res_ev, h->res_stream) != hipSuccess) {
        set_err(h, "resident host-I/O step: event record");
        return PMENV_ERR_HIP;
    }
    h->res_live = true;
    h->res_p = p;
    h->res_io = io;
    return PMENV_OK;
}

// post the call's tag (its inputs are in the staging: stored before, released with the tag) and
// spin on the completion words; a workgroup that exited idle before it saw the tag is relaunched
int res_step(pmenv* h, const StepParams& p, const HostIO& io) {
    const bool same = h->res_live && memcmp(&h->res_p, &p, sizeof p) == 0 &&
                      h->res_io.close_in == io.close_in && h->res_io.chan == io.chan &&
                      h->res_io.value_out == io.value_out && h->res_io.done == io.done;
    if (!same) res_stop(h);
    if (!h->res_live || hipEventQuery(h->res_ev) == hipSuccess)
        if (const int rc = res_launch(h, p, io)) return rc;
    __atomic_store_n(hio_host<uint32_t>(h, kHioGo), io.seq, __ATOMIC_RELEASE);
    const volatile uint32_t* done = hio_host<volatile uint32_t>(h, kHioDone);
    const int B = h->cfg.num_envs;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t it = 1;; ++it) {
        int b = 0;
        while (b < B && done[b] == io.seq) ++b;
        if (b == B) {
            __atomic_thread_fence(__ATOMIC_ACQUIRE);        // the outputs are read after the words
            return PMENV_OK;
        }
        if ((it & 1023u) == 0u) {
            const hipError_t q = hipEventQuery(h->res_ev);
            if (q == hipSuccess) {                          // exited idle as the tag arrived: relaunch
                if (const int rc = res_launch(h, p, io)) return rc;
            } else if (q != hipErrorNotReady) {
                set_err(h, "step_host_resident_kernel: %s", hipGetErrorString(q));
                return PMENV_ERR_HIP;
            }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
                set_err(h, "step_host_resident_kernel: no completion within 2 s");
                return PMENV_ERR_HIP;
            }
        }
    }
}
}  // namespace

extern "C" {

int pmenv_step_host(pmenv* h, const float* action, const float* prices, float* obs, float* reward, double* value,
                    double* ret, float* weights, hipStream_t stream) {
    if (!h) return PMENV_ERR_ARG;
    if (!action || !prices) { set_err(h, "host step: action and prices are required"); return PMENV_ERR_ARG; }
    DeviceGuard g(h->device);
    if (capturing(stream)) {          // the host waits on the kernel's words: nothing runs under capture
        set_err(h, "pmenv_step_host is not graph-capturable (the stream is being captured)");
        return PMENV_ERR_ARG;
    }
    if (const int rc = hio_ensure(h)) return rc;
    // the resident workgroup (no launch per call) for a few envs when none of this handle's own
    // device work can be pending (what the call would otherwise be ordered after on `stream`);
    // else one launch on `stream`
    // (dev_pending: this handle enqueued device work since its last synchronous call — the
    // ordering a launch on `stream` gives; hipStreamQuery would cost ~9 us per call)
    const bool resident = h->cfg.num_envs <= kResMaxEnvs && !h->dev_pending;
    const pmenv_cfg& c = h->cfg;
    const size_t B = (size_t)c.num_envs, BN = B * (size_t)c.num_assets;
    memcpy(hio_host<float>(h, kHioAct), action, BN * 4);
    memcpy(hio_host<float>(h, kHioPri), prices, BN * 4);
    if (obs) hio_gather_closes(h, obs);
    if (const int rc = flat1_invalidate(h, stream)) return rc;   // the snapshot / halos go stale
    StepParams p = base_params(h);
    p.action = hio_dev<float>(h, kHioAct);
    p.prices = hio_dev<float>(h, kHioPri);
    p.reward = hio_dev<float>(h, kHioRew);
    p.ret = hio_dev<double>(h, kHioRet);
    p.weights = hio_dev<float>(h, kHioW);
    HostIO io;
    io.close_in = hio_dev<float>(h, kHioClose);
    io.chan = obs ? hio_dev<float>(h, kHioChan) : nullptr;
    io.value_out = hio_dev<double>(h, kHioVal);
    io.done = hio_dev<uint32_t>(h, kHioDone);
    io.seq = h->hio_seq = h->hio_seq + 1u == 0u ? 1u : h->hio_seq + 1u;
    if (resident) {
        if (const int rc = res_step(h, p, io)) return rc;
    } else {
        step_surface_host_kernel<<<c.num_envs, kBlock, h->lds_surface, stream>>>(p, io);
        if (const int rc = hio_sync(h, stream, "step_surface_host_kernel")) return rc;
        h->dev_pending = false;                     // everything before it on `stream` has run
    }
    if (obs) hio_scatter_channel(h, obs);
    if (reward) memcpy(reward, hio_host<float>(h, kHioRew), B * 4);
    if (ret) memcpy(ret, hio_host<double>(h, kHioRet), B * 8);
    if (value) memcpy(value, hio_host<double>(h, kHioVal), B * 8);
    if (weights) memcpy(weights, hio_host<float>(h, kHioW), BN * 4);
    return PMENV_OK;
}

int pmenv_reset_host(pmenv* h, float* obs, double* value, hipStream_t stream) {
    if (!h) return PMENV_ERR_ARG;
    DeviceGuard g(h->device);
    if (capturing(stream)) {
        set_err(h, "pmenv_reset_host is not graph-capturable (the stream is being captured)");
        return PMENV_ERR_ARG;
    }
    if (const int rc = hio_ensure(h)) return rc;
    if (obs) hio_gather_closes(h, obs);
    if (const int rc = flat1_invalidate(h, stream)) return rc;
    StepParams p = base_params(h);
    HostIO io;
    io.close_in = hio_dev<float>(h, kHioClose);
    io.chan = obs ? hio_dev<float>(h, kHioChan) : nullptr;
    io.value_out = hio_dev<double>(h, kHioVal);
    io.done = hio_dev<uint32_t>(h, kHioDone);
    io.seq = h->hio_seq = h->hio_seq + 1u == 0u ? 1u : h->hio_seq + 1u;
    reset_kernel<<<h->cfg.num_envs, kBlock, 0, stream>>>(p, nullptr, nullptr, io);
    if (const int rc = hio_sync(h, stream, "reset_kernel (host I/O)")) return rc;
    h->dev_pending = false;
    if (obs) hio_scatter_channel(h, obs);
    if (value) memcpy(value, hio_host<double>(h, kHioVal), (size_t)h->cfg.num_envs * 8);
    return PMENV_OK;
}

double* pmenv_value(pmenv* h) { return h ? h->value : nullptr; }
float* pmenv_ring(pmenv* h) { return h ? h->ring : nullptr; }
int32_t* pmenv_counter(pmenv* h) { return h ? h->k : nullptr; }
size_t pmenv_state_bytes(const pmenv* h) { return h ? h->state_bytes : 0; }

const char* pmenv_step_path(const pmenv* h) {
    if (!h) return "";
    static thread_local char out[512];
    step_plan_describe(*h, h->cfg, (h->device_seq ? kDescribeFlatSeq : 0) | (h->relay_dseq ? kDescribeRelaySeq : 0),
                       out, sizeof out);
    return out;
}

const char* pmenv_step_path_for(const pmenv_cfg* cfg, int32_t path, int32_t detail) {
    static thread_local char out[512];
    out[0] = 0;
    if (cfg) step_plan_path_for(*cfg, path, detail != 0, out, sizeof out);
    return out;
}

int pmenv_get_state(pmenv* h, void* dst, hipStream_t stream) {
    if (!h || !dst) return PMENV_ERR_ARG;
    h->dev_pending = true;                          // device work of this handle may be in flight
    DeviceGuard g(h->device);
    hipError_t e = hipMemcpyAsync(dst, h->state, h->state_bytes, hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) { set_err(h, "get_state: %s", hipGetErrorString(e)); return PMENV_ERR_HIP; }
    return PMENV_OK;
}

int pmenv_set_state(pmenv* h, const void* src, hipStream_t stream) {
    if (!h || !src) return PMENV_ERR_ARG;
    h->dev_pending = true;                          // device work of this handle may be in flight
    DeviceGuard g(h->device);
    if (const int rc = flat1_invalidate(h, stream)) return rc;
    hipError_t e = hipMemcpyAsync(h->state, src, h->state_bytes, hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) { set_err(h, "set_state: %s", hipGetErrorString(e)); return PMENV_ERR_HIP; }
    return PMENV_OK;
}

int pmenv_window_written(pmenv* h, const float* obs, hipStream_t stream) {
    if (!h) return PMENV_ERR_ARG;
    h->dev_pending = true;                          // device work of this handle may be in flight
    (void)obs;                                 // any window: the halo is dropped whichever it was
    DeviceGuard g(h->device);
    return flat1_invalidate(h, stream, kInvalHalo);
}

int pmenv_state_written(pmenv* h, hipStream_t stream) {
    if (!h) return PMENV_ERR_ARG;
    h->dev_pending = true;                          // device work of this handle may be in flight
    DeviceGuard g(h->device);
    return flat1_invalidate(h, stream, kInvalSnap | kInvalHalo);
}

int pmenv_nonfinite_count(pmenv* h, uint64_t* out, hipStream_t stream) {
    if (!h || !out) return PMENV_ERR_ARG;
    h->dev_pending = true;                          // device work of this handle may be in flight
    DeviceGuard g(h->device);
    unsigned long long v = 0;
    hipError_t e = hipMemcpyAsync(&v, h->nonfinite, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) { set_err(h, "nonfinite_count: %s", hipGetErrorString(e)); return PMENV_ERR_HIP; }
    *out = v;
    return PMENV_OK;
}

int pmenv_synth_series(float* series, int32_t T, int32_t B, int32_t N, int64_t env_offset, uint64_t seed,
                       float sigma, hipStream_t stream) {
    if (!series || T < 1 || B < 1 || N < 1 || ((uintptr_t)series & 15u)) return PMENV_ERR_ARG;
    const int64_t threads = (int64_t)B * N;
    synth_series_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, stream>>>(
        reinterpret_cast<f4*>(series), T, B, N, env_offset, seed, (double)sigma);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int pmenv_synth_actions(float* actions, int32_t T, int32_t B, int32_t N, int64_t env_offset, uint64_t seed,
                        hipStream_t stream) {
    if (!actions || T < 1 || B < 1 || N < 1) return PMENV_ERR_ARG;
    const int64_t threads = (int64_t)T * B;
    synth_actions_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, stream>>>(actions, T, B, N, env_offset, seed);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int pmenv_window_init(float* obs, const float* series, int32_t B, int32_t N, int32_t W, int32_t F,
                      hipStream_t stream) {
    if (!obs || !series || B < 1 || N < 1 || W < 1 || F != 5 || ((uintptr_t)series & 15u)) return PMENV_ERR_ARG;
    const int64_t threads = (int64_t)B * N * W;
    window_init_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, stream>>>(
        obs, reinterpret_cast<const f4*>(series), B, N, W, F);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int pmenv_window_init_days(float* obs, const float* series, int32_t T, int32_t N, int32_t F, const int32_t* start,
                           int32_t B, int32_t W, hipStream_t stream) {
    if (!obs || !series || !start || T < 1 || B < 1 || N < 1 || W < 1 || F < 2) return PMENV_ERR_ARG;
    const int64_t threads = (int64_t)B * N * W;
    window_init_days_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, stream>>>(obs, series, T, N, F, start, B, W);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

// Horizon split of the tiled GAE scan: used when the B / 64 env blocks leave CUs idle (few
// envs, long horizons). Round 4: one pass (gae_lookback_kernel, 64- or 128-day chunks, every chunk
// composing the later chunks' published maps) in place of the round-3 maps + apply passes
// (gae_chunk_kernel, now in the tools build).
namespace {
// chunk length S = NW x U days: 8 waves x 16 days where that still makes 128 workgroups, else
// 8 x 8 (fewer composes per chunk against fewer workgroups). T x B = 4,096 x 512: 9.85 us for
// 128-day chunks against 12.7 for 64-day; 16,384 x 64: 10.3 vs 11.2; 2,048 x 4,096: 31.5 vs
// 32.4; 1,000 x 200 (32 workgroups): 8.7 vs 7.7 (profiles/ab_r04/gae_geom_r04h.err)
int gae_lb_seg(int32_t T, int32_t B) {
    const int64_t wg16 = (int64_t)((T + 127) / 128) * ((B + 63) / 64);
    return wg16 >= 128 ? 128 : 64;
}
int gae_lb_chunks(int32_t T, int32_t B) {
    // from 8,192 envs (128 workgroups) the one-pass tile with nt stores wins: 2,048 x 8,192
    // 59.0 vs 74.2 us for the round-3 split (profiles/rows_r03af/rows_r03af.json)
    if (B >= 8192 || T < 512) return 0;
    if ((size_t)(T + 1) * (size_t)B * 4u >= (1ull << 31)) return 0;
    const int seg = gae_lb_seg(T, B);
    return (T + seg - 1) / seg;
}
// the look-back flags' epochs: a process-wide counter from a clock-mixed start, so a flag word
// left in a reused workspace (an older epoch) or garbage (2^-64) never passes for this call's
std::atomic<uint64_t> g_gae_epoch{0};
uint64_t gae_next_epoch() {
    uint64_t e = g_gae_epoch.load();
    if (e == 0) {
        const uint64_t seed = ((uint64_t)std::chrono::steady_clock::now().time_since_epoch().count() *
                               0x9E3779B97F4A7C15ull) | 1ull;
        g_gae_epoch.compare_exchange_strong(e, seed);
    }
    return g_gae_epoch.fetch_add(1) + 1;
}

// The one place that decides which GAE kernel a call takes (pmenv_gae: workspace = false;
// pmenv_gae_ex: whether the caller's scratch is usable); pmenv_gae_path names it.
enum gae_kind { kGaeLoop, kGaeScan, kGaeTile16, kGaeTile8, kGaeTile8Occ8, kGaeLb8, kGaeLb16 };
const char* const kGaeNames[] = {"gae_kernel",
                                 "gae_scan_kernel",
                                 "gae_tile_kernel<8,16,1,2>",
                                 "gae_tile_kernel<8,8>",
                                 "gae_tile_kernel<8,8,8,2>",
                                 "gae_lookback_kernel<8,8>",
                                 "gae_lookback_kernel<8,16>"};
gae_kind gae_plan(int32_t T, int32_t B, bool workspace) {
    if (workspace && gae_lb_chunks(T, B)) return gae_lb_seg(T, B) == 128 ? kGaeLb16 : kGaeLb8;
    // measured on MI355X (tools/bench_rows.py, profiles/rows_r01.json): the tiled scan
    // beats the per-env loop 2.7x at T = 256 x B = 65536 and 14x at 2048 x 8192; the
    // wave-per-env scan only for a handful of envs with long horizons
    const bool fits = (size_t)(T + 1) * (size_t)B * 4u < (1ull << 31);   // gae_tile_kernel's buffer offsets
    const bool scan = B < 64 && T >= 256;
    const bool tile = fits && !scan;
    const int U = B >= 16384 ? 8 : 16;           // steps per lane and segment
    // many envs and at least four 64-day segments: the tile held to 64 VGPRs (8 waves per
    // SIMD, so a 65,536-env rollout's 1,024 workgroups are resident at once; the same bits):
    // 56.7 vs 58.5 us at 256 x 65,536, 110.1 vs 114.7 at 512 x 65,536; slower below 65,536
    // envs or 256 days (profiles/ab_r02/gae_occ8_r02zl.json)
    // adv / ret are written once and read by the learner later: nt stores where they measured
    // faster (the same bits): 62.3 -> 45.7 us at 256 x 65,536, 9.0 -> 8.4 at 256 x 4,096,
    // 80.2 -> 58.9 at 2,048 x 8,192 on the tile; at 256 x 16,384 (the U = 8 tile, a cache-
    // resident rollout) 14.1 vs 14.5, so that form keeps plain stores
    // (profiles/rows_r03ad/rows_nt2.json)
    if (tile && U == 8 && B >= 65536 && T >= 256) return kGaeTile8Occ8;
    if (tile && U == 16) return kGaeTile16;
    if (tile) return kGaeTile8;
    return scan ? kGaeScan : kGaeLoop;
}
bool gae_work_usable(int32_t T, int32_t B, const void* work, size_t work_bytes) {
    return work && work_bytes >= pmenv_gae_workspace(T, B) && !((uintptr_t)work & 7u);
}
}  // namespace

size_t pmenv_gae_workspace(int32_t T, int32_t B) {
    const int n = (T < 1 || B < 1) ? 0 : gae_lb_chunks(T, B);
    return n ? ((size_t)2 * n * B + (size_t)n * ((B + 63) / 64)) * sizeof(double) : 0;
}

const char* pmenv_gae_path(int32_t T, int32_t B, size_t work_bytes, int work_aligned) {
    if (T < 1 || B < 1) return "";
    return kGaeNames[gae_plan(T, B, work_aligned && work_bytes >= pmenv_gae_workspace(T, B))];
}

int pmenv_gae(const float* rewards, const float* values, const uint8_t* dones, float* adv, float* ret, int32_t T,
              int32_t B, float gamma, float lam, hipStream_t stream) {
    if (!rewards || !values || !adv || !ret || T < 1 || B < 1) return PMENV_ERR_ARG;
    int rc = PMENV_OK;
    if (pmenv_tools::gae(rewards, values, dones, adv, ret, T, B, gamma, lam, stream, &rc)) return rc;
    switch (gae_plan(T, B, false)) {
    case kGaeTile8Occ8:
        gae_tile_kernel<8, 8, 8, 2><<<(B + 63) / 64, 512, 0, stream>>>(rewards, values, dones, adv, ret, T, B, gamma,
                                                                      lam);
        break;
    case kGaeTile16:
        gae_tile_kernel<8, 16, 1, 2><<<(B + 63) / 64, 512, 0, stream>>>(rewards, values, dones, adv, ret, T, B, gamma,
                                                                       lam);
        break;
    case kGaeTile8:
        gae_tile_kernel<8, 8><<<(B + 63) / 64, 512, 0, stream>>>(rewards, values, dones, adv, ret, T, B, gamma,
                                                                lam);
        break;
    case kGaeScan:
        gae_scan_kernel<<<(B + 3) / 4, 256, 0, stream>>>(rewards, values, dones, adv, ret, T, B, gamma, lam);
        break;
    default:
        gae_kernel<<<(B + 255) / 256, 256, 0, stream>>>(rewards, values, dones, adv, ret, T, B, gamma, lam);
        break;
    }
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int pmenv_gae_ex(const float* rewards, const float* values, const uint8_t* dones, float* adv, float* ret, int32_t T,
                 int32_t B, float gamma, float lam, double* work, size_t work_bytes, hipStream_t stream) {
    if (!rewards || !values || !adv || !ret || T < 1 || B < 1) return PMENV_ERR_ARG;
    int rc = PMENV_OK;
    if (pmenv_tools::gae(rewards, values, dones, adv, ret, T, B, gamma, lam, stream, &rc)) return rc;
    const gae_kind kind = gae_plan(T, B, gae_work_usable(T, B, work, work_bytes));
    // the look-back's epoch is a kernel argument chosen here: a captured call would replay it
    // on the same workspace, whose flags then already carry it, and a consumer could compose
    // the previous replay's maps. The tile, scan and loop kernels keep no cross-call state.
    if ((kind != kGaeLb8 && kind != kGaeLb16) || capturing(stream))
        return pmenv_gae(rewards, values, dones, adv, ret, T, B, gamma, lam, stream);
    const int n = gae_lb_chunks(T, B), neb = (B + 63) / 64;
    uint64_t* flags = reinterpret_cast<uint64_t*>(work + (size_t)2 * n * B);
    if (kind == kGaeLb16)
        gae_lookback_kernel<8, 16><<<(unsigned)(n * neb), 512, 0, stream>>>(rewards, values, dones, adv, ret, T, B,
                                                                          gamma, lam, n, work, flags, gae_next_epoch());
    else
        gae_lookback_kernel<8, 8><<<(unsigned)(n * neb), 512, 0, stream>>>(rewards, values, dones, adv, ret, T, B,
                                                                         gamma, lam, n, work, flags, gae_next_epoch());
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

size_t pmenv_moments_workspace(void) { return (size_t)kMomBlocks * 2 * sizeof(double); }

int pmenv_moments(const float* x, int64_t n, double* out, double* work, hipStream_t stream) {
    if ((!x && n > 0) || !out || !work || n < 0) return PMENV_ERR_ARG;
    const int64_t want = (n + kMomBlock * 16 - 1) / (kMomBlock * 16);   // >= 16 floats per thread
    const int blocks = (int)(want < 1 ? 1 : (want > kMomBlocks ? kMomBlocks : want));
    moments_partial_kernel<<<blocks, kMomBlock, 0, stream>>>(x, n, work);
    moments_final_kernel<<<1, kMomBlock, 0, stream>>>(blocks, n, work, out);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

// ---- the feature pipeline: ffd_plan.h holds the weights and the geometry, features.h the kernels
int pmenv_ffd_weights(double d, double thres, int32_t T, float* taps, int32_t cap, int32_t* width) {
    return ffd_weights(d, thres, T, taps, cap, width);
}

const char* pmenv_ffd_path(int32_t T, int32_t C, int32_t max_width) {
    thread_local char text[160];
    ffd_plan_describe(ffd_plan(T, C, max_width), text, sizeof(text));
    return text;
}

int pmenv_ffd_apply(const float* x, int32_t T, int32_t C, const float* taps, const int32_t* width, int32_t max_width,
                    float* out, hipStream_t stream) {
    if (!x || !width || !out || (max_width > 0 && !taps)) return PMENV_ERR_ARG;
    if (((uintptr_t)x | (uintptr_t)taps | (uintptr_t)width | (uintptr_t)out) & 3u) return PMENV_ERR_ALIGN;
    const FfdPlan plan = ffd_plan(T, C, max_width);
    if (!plan.ok) return PMENV_ERR_ARG;
    // out must overlap neither x nor the tap table: a lane reads rows other lanes write
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)(T - max_width) * (size_t)C * sizeof(float);
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (size_t)T * (size_t)C * sizeof(float);
    const uintptr_t w0 = (uintptr_t)taps, w1 = w0 + (size_t)max_width * (size_t)C * sizeof(float);
    if ((o0 < x1 && x0 < o1) || (max_width > 0 && o0 < w1 && w0 < o1)) return PMENV_ERR_ARG;
    ffd_apply_kernel<kFfdRB, kFfdJB><<<dim3(plan.grid_x, plan.grid_y), plan.block, 0, stream>>>(
        x, taps, width, out, T, C, max_width, plan.cw_log2);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

size_t pmenv_scale_workspace(int32_t T, int32_t C) { return scale_workspace(T, C); }

int pmenv_scale_fit(const float* x, int32_t T, int32_t C, int32_t method, double* stats, double* work,
                    size_t work_bytes, hipStream_t stream) {
    const int64_t chunks = scale_chunks(T, C);
    if (!x || !stats || !work || chunks < 1 || (method != PMENV_SCALE_MINMAX && method != PMENV_SCALE_STANDARD) ||
        work_bytes < scale_workspace(T, C))
        return PMENV_ERR_ARG;
    if (((uintptr_t)x & 3u) || (((uintptr_t)stats | (uintptr_t)work) & 7u)) return PMENV_ERR_ALIGN;
    const dim3 grid((unsigned)((C + 63) / 64), (unsigned)chunks);
    const unsigned fin = (unsigned)((C + 255) / 256);
    if (method == PMENV_SCALE_MINMAX) {
        scale_partial_kernel<0><<<grid, 256, 0, stream>>>(x, T, C, stats, work);
        scale_final_kernel<0><<<fin, 256, 0, stream>>>((int)chunks, C, work, stats);
    } else {                                          // two passes: the mean, then the squares about it
        scale_partial_kernel<1><<<grid, 256, 0, stream>>>(x, T, C, stats, work);
        scale_final_kernel<1><<<fin, 256, 0, stream>>>((int)chunks, C, work, stats);
        scale_partial_kernel<2><<<grid, 256, 0, stream>>>(x, T, C, stats, work);
        scale_final_kernel<2><<<fin, 256, 0, stream>>>((int)chunks, C, work, stats);
    }
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int pmenv_scale_apply(const float* x, int32_t T, int32_t C, int32_t method, const double* stats, float* y,
                      hipStream_t stream) {
    if (!x || !stats || !y || T < 1 || C < 1 || (method != PMENV_SCALE_MINMAX && method != PMENV_SCALE_STANDARD) ||
        ((int64_t)C + 63) / 64 > 65535)
        return PMENV_ERR_ARG;
    if ((((uintptr_t)x | (uintptr_t)y) & 3u) || ((uintptr_t)stats & 7u)) return PMENV_ERR_ALIGN;
    const dim3 grid((unsigned)(((int64_t)T + 31) / 32), (unsigned)((C + 63) / 64));
    scale_apply_kernel<<<grid, 256, 0, stream>>>(x, T, C, method == PMENV_SCALE_STANDARD, stats, y);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

// ---- the search for the orders of differencing: adf_plan.h holds the lag rule, the p-value and
// the geometry, adf.h the kernels
int pmenv_ffd_table(const double* d, double thres, int32_t T, int32_t C, int32_t cap, float* taps, int32_t* width,
                    hipStream_t stream) {
    if (!d || !width || T < 2 || C < 1 || cap < 0 || (cap > 0 && !taps) || !(thres >= 0.0) || !isfinite(thres))
        return PMENV_ERR_ARG;
    if (((uintptr_t)d & 7u) || (((uintptr_t)taps | (uintptr_t)width) & 3u)) return PMENV_ERR_ALIGN;
    const unsigned grid = (unsigned)(((int64_t)C + kAdfTableBlock - 1) / kAdfTableBlock);
    ffd_table_kernel<<<grid, kAdfTableBlock, 0, stream>>>(d, thres, T, C, cap, taps, width);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int32_t pmenv_adf_maxlag(int64_t n, int32_t maxlag) { return (int32_t)adf_maxlag(n, maxlag); }

double pmenv_adf_pvalue(double stat) { return adf_pvalue(stat); }

size_t pmenv_adf_workspace(int32_t R, int32_t C, int32_t maxlag) { return adf_plan(R, C, C, maxlag).work_bytes; }

const char* pmenv_adf_path(int32_t R, int32_t C, int32_t maxlag) {
    thread_local char text[256];
    adf_plan_describe(adf_plan(R, C, C, maxlag), text, sizeof(text));
    return text;
}

int pmenv_adf(const float* y, int32_t R, int32_t C, int32_t ld, const int32_t* first, int32_t maxlag, int32_t autolag,
              double* stat, double* pvalue, int32_t* usedlag, int32_t* nobs, int32_t* status, void* work,
              size_t work_bytes, hipStream_t stream) {
    if (!y || !stat || !pvalue || !usedlag || !nobs || !status) return PMENV_ERR_ARG;
    const AdfPlan plan = adf_plan(R, C, ld, maxlag);
    if (!plan.ok || !work || ((uintptr_t)work & 7u) || work_bytes < plan.work_bytes) return PMENV_ERR_ARG;
    if ((((uintptr_t)y | (uintptr_t)first | (uintptr_t)usedlag | (uintptr_t)nobs | (uintptr_t)status) & 3u) ||
        (((uintptr_t)stat | (uintptr_t)pvalue) & 7u))
        return PMENV_ERR_ALIGN;
    adf_sums_kernel<<<plan.sums_grid, plan.sums_block, 0, stream>>>(y, first, R, C, ld, maxlag, plan.rec,
                                                                    (double*)work);
    adf_solve_kernel<<<plan.solve_grid, plan.solve_block, plan.solve_lds, stream>>>(
        y, first, R, C, ld, maxlag, autolag != 0, plan.kcap, plan.rec, (const double*)work, stat, pvalue, usedlag, nobs,
        status);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int pmenv_adf_search_update(const double* pvalue, const double* stat, const int32_t* adf_status, double thres,
                            int32_t C, double* low, double* high, double* d_opt, int32_t* active, int32_t* evals,
                            int32_t* status, double* last, double* d, hipStream_t stream) {
    if (!low || !high || !d_opt || !active || !evals || !status || !d || C < 1 || !(thres > 0.0) ||
        (pvalue && (!stat || !adf_status)))
        return PMENV_ERR_ARG;
    if ((((uintptr_t)pvalue | (uintptr_t)stat | (uintptr_t)low | (uintptr_t)high | (uintptr_t)d_opt | (uintptr_t)last |
          (uintptr_t)d) & 7u) ||
        (((uintptr_t)adf_status | (uintptr_t)active | (uintptr_t)evals | (uintptr_t)status) & 3u))
        return PMENV_ERR_ALIGN;
    adf_search_update_kernel<<<(unsigned)(((int64_t)C + 255) / 256), 256, 0, stream>>>(
        pvalue, stat, adf_status, thres, C, low, high, d_opt, active, evals, status, last, d);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

// ---- the technical indicators: ind_plan.h holds the ops' parameters and every decision,
// indicators.h the kernels; the four entry points read the same IndPlan
int pmenv_ind_layout(const pmenv_ind_op* ops, int32_t n_ops, int32_t* n_out, int32_t* lookback) {
    return ind_layout(ops, n_ops, n_out, lookback);
}

size_t pmenv_ind_workspace(int32_t T, int32_t N, const pmenv_ind_op* ops, int32_t n_ops) {
    const IndPlan plan = ind_plan(T, N, ops, n_ops, pmenv_tools::ind_form());
    return plan.ok ? plan.work_bytes : 0;
}

const char* pmenv_ind_path(int32_t T, int32_t N, const pmenv_ind_op* ops, int32_t n_ops) {
    thread_local char text[512];
    ind_plan_describe(ind_plan(T, N, ops, n_ops, pmenv_tools::ind_form()), text, sizeof(text));
    return text;
}

int pmenv_ind_apply(const float* bars, int32_t T, int32_t N, int32_t C, const int32_t chan[5], const pmenv_ind_op* ops,
                    int32_t n_ops, float* out, int32_t ldo, int32_t col0, void* work, size_t work_bytes,
                    hipStream_t stream) {
    if (!bars || !chan || !out || C < 1) return PMENV_ERR_ARG;
    const IndPlan plan = ind_plan(T, N, ops, n_ops, pmenv_tools::ind_form());
    if (!plan.ok || col0 < 0 || (int64_t)col0 + plan.K > ldo) return PMENV_ERR_ARG;
    for (int i = 0; i < 5; ++i)
        if (((plan.need >> i) & 1u) && (chan[i] < 0 || chan[i] >= C)) return PMENV_ERR_ARG;
    if (plan.work_bytes > 0 && (!work || work_bytes < plan.work_bytes || ((uintptr_t)work & 7u))) return PMENV_ERR_ARG;
    if (((uintptr_t)bars | (uintptr_t)out) & 3u) return PMENV_ERR_ALIGN;
    const size_t R = (size_t)(T - plan.L);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + R * (size_t)N * (size_t)ldo * sizeof(float);
    const uintptr_t x0 = (uintptr_t)bars, x1 = x0 + (size_t)T * (size_t)N * (size_t)C * sizeof(float);
    if (o0 < x1 && x0 < o1) return PMENV_ERR_ARG;

    for (int w = 0; w < plan.n_walks; ++w) {
        const IndWalk& wk = plan.walk[w];
        IndScanArgs a;
        memset(&a, 0, sizeof(a));
        a.bars = bars;
        a.out = out;
        a.rec = (double*)work;
        a.T = T; a.N = N; a.C = C; a.ldo = ldo; a.L = plan.L;
        for (int i = 0; i < 5; ++i) a.ch[i] = chan[i];
        a.mask = wk.mask;
        a.need = wk.need;
        for (int k = 0; k < kIndKinds; ++k) {
            for (int j = 0; j < 3; ++j) a.p[k][j] = wk.p[k][j];
            a.col[k] = col0 + wk.col[k];
        }
        a.seg_len = plan.seg_len;
        a.n_seg = plan.n_seg;
        if (plan.form == kIndSplit) {
            for (int i = 0; i < kIndSlots; ++i) a.apow[i] = ind_pow(ind_slot_coef(wk, i), plan.seg_len);
            const dim3 all(plan.scan_grid, (unsigned)plan.n_seg), rest(plan.scan_grid, (unsigned)(plan.n_seg - 1));
            ind_scan_split_kernel<1><<<all, 64, 0, stream>>>(a);
            if (wk.mask & kIndLevel2Mask) {             // the level-2 kinds alone: their level 1, then their level 2
                IndScanArgs b = a;
                b.mask = wk.mask & kIndLevel2Mask;
                ind_scan_split_kernel<2><<<rest, 64, 0, stream>>>(b);
            }
            ind_scan_split_kernel<3><<<rest, 64, 0, stream>>>(a);
        } else {
            ind_scan_seq_kernel<<<plan.scan_grid, 64, 0, stream>>>(a);
        }
    }
    for (int w = 0; w < plan.n_window; ++w) {
        const IndWindowOp& op = plan.window[w];
        IndWinArgs a;
        memset(&a, 0, sizeof(a));
        a.bars = bars;
        a.out = out;
        a.fastk = (double*)((char*)work + plan.fastk_off);
        a.T = T; a.N = N; a.C = C; a.ldo = ldo; a.L = plan.L;
        for (int i = 0; i < 5; ++i) a.ch[i] = chan[i];
        a.col = col0 + op.col;
        for (int j = 0; j < 3; ++j) a.p[j] = op.p[j];
        a.f[0] = op.f[0];
        a.f[1] = op.f[1];
        if (op.kind == PMENV_IND_BBANDS) {
            ind_window_kernel<PMENV_IND_BBANDS><<<plan.window_grid, kIndWindowBlock, 0, stream>>>(a);
        } else if (op.kind == PMENV_IND_CCI) {
            ind_window_kernel<PMENV_IND_CCI><<<plan.window_grid, kIndWindowBlock, 0, stream>>>(a);
        } else {
            ind_fastk_kernel<<<plan.fastk_grid, kIndWindowBlock, 0, stream>>>(a);
            ind_window_kernel<PMENV_IND_STOCH><<<plan.window_grid, kIndWindowBlock, 0, stream>>>(a);
        }
    }
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

// ---- the sample gathers: replay_plan.h decides the kernel and its geometry, the entry points
// validate, plan and launch; pmenv_replay_path names the plan
const char* pmenv_replay_path(int32_t kind, int32_t N, int32_t F, int32_t W, int32_t n, int32_t S, int32_t aligned,
                              int32_t cus) {
    thread_local char text[160];
    text[0] = 0;
    const bool has_n = kind == PMENV_REPLAY_NSTEP || kind == PMENV_REPLAY_SEQ;
    if (N < 1 || F < 2 || W < 1 || S < 1 || (has_n && n < 1) || aligned < 0 || aligned > 3) return text;
    const ReplayPlan plan = replay_plan(kind, N, F, W, n, S, aligned, cus > 0 ? cus : device_cus());
    replay_plan_describe(kind, plan, text, sizeof(text));
    return text;
}

int pmenv_replay_gather(const float* series, int32_t T, int32_t N, int32_t F, int32_t W, const int32_t* days,
                        const float* actions, const float* rewards, int32_t H, int32_t B, const int32_t* h0,
                        const int32_t* env, int32_t S, float* s, float* s_next, float* a_out, float* r_out,
                        hipStream_t stream) {
    if (!series || !days || !actions || !rewards || !h0 || !env || !s || !s_next || !a_out || !r_out || T < 1 ||
        N < 1 || F < 2 || W < 1 || H < W + 1 || B < 1 || S < 1)
        return PMENV_ERR_ARG;
    int rc = PMENV_OK;
    if (pmenv_tools::replay_gather(series, T, N, F, W, days, actions, rewards, H, B, h0, env, S, s, s_next, a_out,
                                   r_out, stream, &rc))
        return rc;
    const ReplayPlan plan =
        replay_plan(PMENV_REPLAY_ONE_STEP, N, F, W, 1, S, replay_aligned(s, s_next, series), device_cus());
    const dim3 grid(plan.grid_x, plan.grid_y);
    switch (plan.form) {
    case kReplayF5p:
        with_const<2, 4, 8>(plan.ppt, [&](auto ppt) {
            replay_gather_f5p_kernel<decltype(ppt)::value, 2><<<grid, plan.block, plan.lds_bytes, stream>>>(
                series, T, N, W, days, actions, rewards, H, B, h0, env, S, s, s_next, a_out, r_out, plan.R,
                make_fastdiv((uint32_t)plan.R), make_fastdiv((uint32_t)(W * F)));
        });
        break;
    case kReplayLds:
        replay_gather_lds_kernel<<<grid, plan.block, plan.lds_bytes, stream>>>(
            series, T, N, F, W, days, actions, rewards, H, B, h0, env, s, s_next, a_out, r_out);
        break;
    case kReplayElem:
        replay_gather_kernel<<<grid, plan.block, 0, stream>>>(series, T, N, F, W, days, actions, rewards, H, B, h0,
                                                             env, S, s, s_next, a_out, r_out);
        break;
    default: return PMENV_ERR_ARG;
    }
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

// ids: row_episode [H] (per_env = false) or env_episode [H, B]; NULL = one episode either way
static int replay_gather_nstep(const float* series, int32_t T, int32_t N, int32_t F, int32_t W, const int32_t* days,
                               const float* actions, const float* rewards, int32_t H, int32_t B, const int32_t* h0,
                               const int32_t* env, int32_t S, const int32_t* ids, bool per_env, int32_t oldest,
                               int32_t count, int32_t n, float gamma, float* s, float* s_next, float* a_out,
                               float* r_out, int32_t* steps, float* discount, hipStream_t stream) {
    if (!series || !days || !actions || !rewards || !h0 || !env || !s || !s_next || !a_out || !r_out || !steps ||
        !discount || T < 1 || N < 1 || F < 2 || W < 1 || H < W + 1 || B < 1 || S < 1 || n < 1 || count < 0 ||
        count > H || oldest < 0 || oldest >= H || !(gamma > 0.0f && gamma <= 1.0f))
        return PMENV_ERR_ARG;
    const NstepRing rg{ids, oldest, count, n, (double)gamma, ids && per_env ? B : 1, ids && per_env ? 1 : 0};
    const ReplayPlan plan =
        replay_plan(PMENV_REPLAY_NSTEP, N, F, W, n, S, replay_aligned(s, s_next, series), device_cus());
    const dim3 grid(plan.grid_x, plan.grid_y);
    switch (plan.form) {
    case kReplayF5p:
        // the plan's kernel, built once per id layout (replay.h ring_ep)
        with_const<2, 4, 8, 12>(plan.ppt, [&](auto ppt) {
            constexpr int kPpt = decltype(ppt)::value;
            auto* kernel = ids && per_env ? replay_nstep_f5p_env_kernel<kPpt, 2> : replay_nstep_f5p_kernel<kPpt, 2>;
            kernel<<<grid, plan.block, plan.lds_bytes, stream>>>(
                series, T, N, W, days, actions, rewards, H, B, h0, env, S, rg, plan.D, s, s_next, a_out, r_out,
                steps, discount, plan.R, make_fastdiv((uint32_t)plan.R), make_fastdiv((uint32_t)(W * F)));
        });
        break;
    case kReplayLds:
        replay_nstep_lds_kernel<<<grid, plan.block, plan.lds_bytes, stream>>>(
            series, T, N, F, W, days, actions, rewards, H, B, h0, env, rg, plan.D, s, s_next, a_out, r_out, steps,
            discount);
        break;
    case kReplayElem:
        replay_nstep_kernel<<<grid, plan.block, 0, stream>>>(series, T, N, F, W, days, actions, rewards, H, B, h0,
                                                            env, S, rg, s, s_next, a_out, r_out, steps, discount);
        break;
    default: return PMENV_ERR_ARG;
    }
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int pmenv_replay_gather_nstep(const float* series, int32_t T, int32_t N, int32_t F, int32_t W, const int32_t* days,
                              const float* actions, const float* rewards, int32_t H, int32_t B, const int32_t* h0,
                              const int32_t* env, int32_t S, const int32_t* row_episode, int32_t oldest,
                              int32_t count, int32_t n, float gamma, float* s, float* s_next, float* a_out,
                              float* r_out, int32_t* steps, float* discount, hipStream_t stream) {
    return replay_gather_nstep(series, T, N, F, W, days, actions, rewards, H, B, h0, env, S, row_episode, false,
                               oldest, count, n, gamma, s, s_next, a_out, r_out, steps, discount, stream);
}

int pmenv_replay_gather_nstep_env(const float* series, int32_t T, int32_t N, int32_t F, int32_t W,
                                  const int32_t* days, const float* actions, const float* rewards, int32_t H,
                                  int32_t B, const int32_t* h0, const int32_t* env, int32_t S,
                                  const int32_t* env_episode, int32_t oldest, int32_t count, int32_t n, float gamma,
                                  float* s, float* s_next, float* a_out, float* r_out, int32_t* steps,
                                  float* discount, hipStream_t stream) {
    return replay_gather_nstep(series, T, N, F, W, days, actions, rewards, H, B, h0, env, S, env_episode, true,
                               oldest, count, n, gamma, s, s_next, a_out, r_out, steps, discount, stream);
}

static int replay_gather_seq(const float* series, int32_t T, int32_t N, int32_t F, int32_t W, const int32_t* days,
                             const float* actions, const float* rewards, int32_t H, int32_t B, const int32_t* h0,
                             const int32_t* env, int32_t S, const int32_t* ids, bool per_env, int32_t oldest,
                             int32_t count, int32_t L, int32_t time_major, float* x, float* a_out, float* r_out,
                             int32_t* length, hipStream_t stream) {
    if (!series || !days || !actions || !rewards || !h0 || !env || !x || !a_out || !r_out || !length || T < 1 ||
        N < 1 || F < 2 || W < 1 || H < W + 1 || B < 1 || S < 1 || L < 1 || count < 0 || count > H || oldest < 0 ||
        oldest >= H)
        return PMENV_ERR_ARG;
    const NstepRing rg{ids, oldest, count, L, 1.0, ids && per_env ? B : 1, ids && per_env ? 1 : 0};
    int policy = -1, lc_knob = 0;
    pmenv_tools::replay_seq_knobs(&policy, &lc_knob);
    const ReplayPlan plan =
        replay_plan(PMENV_REPLAY_SEQ, N, F, W, L, S, replay_aligned(x, x, series), device_cus(), policy, lc_knob);
    switch (plan.form) {
    case kReplayF5p:
        with_const<2, 4, 8, 12>(plan.ppt, [&](auto ppt) {
            with_const<16, 2, 0>(plan.policy, [&](auto nt) {
                constexpr int kPpt = decltype(ppt)::value, kNt = decltype(nt)::value;
                auto* kernel = ids && per_env ? replay_seq_f5p_env_kernel<kPpt, kNt> : replay_seq_f5p_kernel<kPpt, kNt>;
                kernel<<<plan.grid_x, plan.block, plan.lds_bytes, stream>>>(
                        series, T, N, W, days, actions, rewards, H, B, h0, env, S, rg, plan.Lc, plan.nc, time_major,
                        x, a_out, r_out, length, plan.R, make_fastdiv((uint32_t)plan.R),
                        make_fastdiv((uint32_t)(W * F)), make_fastdiv((uint32_t)plan.nc),
                        make_fastdiv((uint32_t)plan.gy));
            });
        });
        break;
    case kReplayElem:
        replay_seq_kernel<<<plan.grid_x, plan.block, 0, stream>>>(series, T, N, F, W, days, actions, rewards, H, B,
                                                                 h0, env, S, rg, time_major, x, a_out, r_out,
                                                                 length);
        break;
    default: return PMENV_ERR_ARG;                         // more workgroups than a grid holds
    }
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int pmenv_replay_gather_seq(const float* series, int32_t T, int32_t N, int32_t F, int32_t W, const int32_t* days,
                            const float* actions, const float* rewards, int32_t H, int32_t B, const int32_t* h0,
                            const int32_t* env, int32_t S, const int32_t* row_episode, int32_t oldest, int32_t count,
                            int32_t L, int32_t time_major, float* x, float* a_out, float* r_out, int32_t* length,
                            hipStream_t stream) {
    return replay_gather_seq(series, T, N, F, W, days, actions, rewards, H, B, h0, env, S, row_episode, false, oldest,
                             count, L, time_major, x, a_out, r_out, length, stream);
}

int pmenv_replay_gather_seq_env(const float* series, int32_t T, int32_t N, int32_t F, int32_t W, const int32_t* days,
                                const float* actions, const float* rewards, int32_t H, int32_t B, const int32_t* h0,
                                const int32_t* env, int32_t S, const int32_t* env_episode, int32_t oldest,
                                int32_t count, int32_t L, int32_t time_major, float* x, float* a_out, float* r_out,
                                int32_t* length, hipStream_t stream) {
    return replay_gather_seq(series, T, N, F, W, days, actions, rewards, H, B, h0, env, S, env_episode, true, oldest,
                             count, L, time_major, x, a_out, r_out, length, stream);
}

// ---- the valid (start, env) pairs of a per-env replay (replay_valid.h)
int pmenv_replay_valid_build(const int32_t* env_episode, int32_t H, int32_t B, int32_t oldest, int32_t count,
                             int32_t need, uint64_t* bits, int64_t* rowsum, hipStream_t stream) {
    if (!env_episode || !rowsum || H < 1 || B < 1 || oldest < 0 || oldest >= H || count < 0 || count > H || need < 1)
        return PMENV_ERR_ARG;
    const int span = count > need ? count - need : 0;
    if (span > 0 && !bits) return PMENV_ERR_ARG;
    if (((uintptr_t)bits | (uintptr_t)rowsum) & 7u) return PMENV_ERR_ALIGN;
    const int WB = (B + 63) / 64;
    if (span > 0) {
        int waves = (WB + kValidWordsPerWave - 1) / kValidWordsPerWave;
        waves = waves < 1 ? 1 : waves > 16 ? 16 : waves;
        valid_bits_kernel<<<(unsigned)span, 64 * waves, 0, stream>>>(env_episode, H, B, oldest, need, WB,
                                                                     (unsigned long long*)bits, (long long*)rowsum);
    }
    valid_scan_kernel<<<1, 1024, 0, stream>>>((long long*)rowsum, span);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int pmenv_replay_valid_select(const uint64_t* bits, const int64_t* rowsum, int32_t H, int32_t B, int32_t oldest,
                              int32_t span, const double* u, int32_t S, int32_t* h0, int32_t* env,
                              hipStream_t stream) {
    if (!rowsum || !u || !h0 || !env || H < 1 || B < 1 || oldest < 0 || oldest >= H || span < 0 || span > H ||
        S < 1 || (span > 0 && !bits))
        return PMENV_ERR_ARG;
    if (((uintptr_t)bits | (uintptr_t)rowsum | (uintptr_t)u) & 7u) return PMENV_ERR_ALIGN;
    valid_select_kernel<<<(unsigned)((S + 3) / 4), 256, 0, stream>>>(
        (const unsigned long long*)bits, (const long long*)rowsum, H, B, oldest, span, u, S, h0, env);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

// ---- the priority tree (prio.h): stateless, every call enqueues a linear chain on `stream`
static bool prio_tree_ok(const void* tree, int64_t leaves) {
    return tree && leaves >= 1 && leaves < ((int64_t)1 << 31);
}

size_t pmenv_prio_tree_bytes(int64_t leaves) {
    if (leaves < 1 || leaves >= ((int64_t)1 << 31)) return 0;
    return prio_layout(leaves).bytes;
}

int pmenv_prio_init(void* tree, int64_t leaves, hipStream_t stream) {
    if (!prio_tree_ok(tree, leaves)) return PMENV_ERR_ARG;
    if ((uintptr_t)tree & 7u) return PMENV_ERR_ALIGN;
    const size_t words = prio_layout(leaves).bytes / 8;
    const size_t blocks = (words + 255) / 256;
    prio_init_kernel<<<(unsigned)(blocks < 4096 ? blocks : 4096), 256, 0, stream>>>((unsigned long long*)tree, words);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

// ep_first / ep_last: pmenv_prio_fill_env's mask of the open range (nullptr: every leaf of it opens)
static int prio_fill(void* tree, int64_t leaves, int64_t close_first, int64_t open_first, int64_t n,
                     const int32_t* ep_first, const int32_t* ep_last, hipStream_t stream) {
    if (!prio_tree_ok(tree, leaves) || n < 0) return PMENV_ERR_ARG;
    if ((uintptr_t)tree & 7u) return PMENV_ERR_ALIGN;
    const int64_t c0 = close_first < 0 ? -1 : close_first, o0 = open_first < 0 ? -1 : open_first;
    if ((c0 >= 0 && c0 + n > leaves) || (o0 >= 0 && o0 + n > leaves)) return PMENV_ERR_ARG;
    if (c0 >= 0 && o0 >= 0 && c0 < o0 + n && o0 < c0 + n && n > 0) return PMENV_ERR_ARG;   // the ranges overlap
    if (n == 0 || (c0 < 0 && o0 < 0)) return PMENV_OK;
    const PrioTree t = prio_layout(leaves);
    char* base = (char*)tree;
    for (int k = 1; k <= t.levels; ++k) {
        const int sh = 6 * k;
        const int64_t cc = c0 < 0 ? 0 : ((c0 + n - 1) >> sh) - (c0 >> sh) + 1;
        const int64_t oc = o0 < 0 ? 0 : ((o0 + n - 1) >> sh) - (o0 >> sh) + 1;
        prio_fill_kernel<<<(unsigned)((cc + oc + 3) / 4), 256, 0, stream>>>(
            (const float*)base, (float*)(base + t.off[0]), (const double*)(base + t.off[k - 1]),
            (double*)(base + t.off[k]), leaves, c0, o0, n, sh, k == 1 ? ep_first : nullptr,
            k == 1 ? ep_last : nullptr);
    }
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int pmenv_prio_fill(void* tree, int64_t leaves, int64_t close_first, int64_t open_first, int64_t n,
                    hipStream_t stream) {
    return prio_fill(tree, leaves, close_first, open_first, n, nullptr, nullptr, stream);
}

int pmenv_prio_fill_env(void* tree, int64_t leaves, int64_t close_first, int64_t open_first, int64_t n,
                        const int32_t* ep_first, const int32_t* ep_last, hipStream_t stream) {
    if (open_first >= 0 && (!ep_first || !ep_last)) return PMENV_ERR_ARG;
    return prio_fill(tree, leaves, close_first, open_first, n, ep_first, ep_last, stream);
}

int pmenv_prio_sample(const void* tree, int64_t leaves, int32_t B, const double* u, int32_t S, float beta,
                      int32_t* leaf_out, int32_t* h0_out, int32_t* env_out, float* weight_out, hipStream_t stream) {
    if (!prio_tree_ok(tree, leaves) || !u || !leaf_out || !h0_out || !env_out || !weight_out || B < 1 || S < 1 ||
        !(beta >= 0.0f) || !std::isfinite(beta))
        return PMENV_ERR_ARG;
    if ((uintptr_t)tree & 7u) return PMENV_ERR_ALIGN;
    prio_sample_kernel<<<(unsigned)((S + 3) / 4), 256, 0, stream>>>((const char*)tree, prio_layout(leaves), B, u, S,
                                                                   leaf_out, h0_out, env_out, weight_out);
    const int wblocks = (S + 1023) / 1024;
    prio_weight_kernel<<<(unsigned)(wblocks < 16 ? wblocks : 16), 1024, 0, stream>>>(
        (const float*)((const char*)tree + kPrioHeaderBytes), leaf_out, weight_out, S, (double)beta);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int pmenv_prio_update(void* tree, int64_t leaves, const int32_t* leaf, const float* td, int32_t S, float alpha,
                      float eps, hipStream_t stream) {
    if (!prio_tree_ok(tree, leaves) || !leaf || !td || S < 1 || !(alpha >= 0.0f) || !std::isfinite(alpha) ||
        !(eps >= 0.0f) || !std::isfinite(eps))
        return PMENV_ERR_ARG;
    if ((uintptr_t)tree & 7u) return PMENV_ERR_ALIGN;
    const PrioTree t = prio_layout(leaves);
    char* base = (char*)tree;
    uint32_t* bits = (uint32_t*)(base + t.off[0]);
    const unsigned tb = (unsigned)((S + 255) / 256), wb = (unsigned)((S + 3) / 4);
    prio_mark_kernel<<<tb, 256, 0, stream>>>(bits, leaves, leaf, S);
    prio_apply_kernel<<<tb, 256, 0, stream>>>((const float*)base, bits, leaves, leaf, td, S, (double)alpha,
                                             (double)eps);
    for (int k = 1; k <= t.levels; ++k)
        prio_refresh_kernel<<<wb, 256, 0, stream>>>((uint32_t*)base, (const float*)(base + t.off[0]),
                                                   (const double*)(base + t.off[k - 1]), (double*)(base + t.off[k]),
                                                   leaves, leaf, td, S, (double)alpha, (double)eps, 6 * k);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int pmenv_rollout_gather(const float* series, int32_t T, int32_t N, int32_t F, int32_t W, const int32_t* start,
                         const float* weights, int32_t T_rec, int32_t B, int32_t ring_mode, const int32_t* t_idx,
                         const int32_t* env, int32_t S, float* s, hipStream_t stream) {
    if (!series || !start || (!weights && T_rec > 0) || !t_idx || !env || !s || T < 1 || N < 1 || F < 2 || W < 1 ||
        T_rec < 0 || B < 1 || S < 1 || ring_mode < 0 || ring_mode > 1)
        return PMENV_ERR_ARG;
    int rc = PMENV_OK;
    if (pmenv_tools::rollout_gather(series, T, N, F, W, start, weights, T_rec, B, ring_mode, t_idx, env, S, s,
                                    stream, &rc))
        return rc;
    const ReplayPlan plan =
        replay_plan(PMENV_REPLAY_ROLLOUT, N, F, W, 1, S, replay_aligned(s, s, series), device_cus());
    switch (plan.form) {
    case kRolloutTile:
        with_const<16, 2>(plan.policy, [&](auto nt) {
            rollout_gather_tile_kernel<decltype(nt)::value><<<plan.grid_x, plan.block, plan.lds_bytes, stream>>>(
                series, T, N, W, start, weights, B, ring_mode, t_idx, env, s, make_fastdiv((uint32_t)N),
                make_fastdiv((uint32_t)(W * F)), make_fastdiv((uint32_t)F));
        });
        break;
    case kRolloutRows:
        rollout_gather_rows_kernel<<<plan.grid_x, plan.block, 0, stream>>>(
            series, T, N, F, W, start, weights, B, ring_mode, t_idx, env, S, s, make_fastdiv((uint32_t)F));
        break;
    default: return PMENV_ERR_ARG;
    }
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

// the per-env form: the lockstep call's plan (form, grid, LDS bytes, store policy), the env kernels
int pmenv_rollout_gather_env(const float* series, int32_t T, int32_t N, int32_t F, int32_t W, const int32_t* first,
                             const int32_t* updates, const float* weights, int32_t carry, int32_t T_rec, int32_t B,
                             int32_t ring_mode, const int32_t* t_idx, const int32_t* env, int32_t S, float* s,
                             hipStream_t stream) {
    if (!series || !first || !updates || !weights || carry < 0 || !t_idx || !env || !s || T < 1 || N < 1 || F < 2 ||
        W < 1 || T_rec < 0 || B < 1 || S < 1 || ring_mode < 0 || ring_mode > 1)
        return PMENV_ERR_ARG;
    const ReplayPlan plan =
        replay_plan(PMENV_REPLAY_ROLLOUT, N, F, W, 1, S, replay_aligned(s, s, series), device_cus());
    switch (plan.form) {
    case kRolloutTile:
        with_const<16, 2>(plan.policy, [&](auto nt) {
            rollout_gather_env_tile_kernel<decltype(nt)::value><<<plan.grid_x, plan.block, plan.lds_bytes, stream>>>(
                series, T, N, W, first, updates, weights, carry, T_rec, B, ring_mode, t_idx, env, s,
                make_fastdiv((uint32_t)N), make_fastdiv((uint32_t)(W * F)), make_fastdiv((uint32_t)F));
        });
        break;
    case kRolloutRows:
        rollout_gather_env_rows_kernel<<<plan.grid_x, plan.block, 0, stream>>>(
            series, T, N, F, W, first, updates, weights, carry, T_rec, B, ring_mode, t_idx, env, S, s,
            make_fastdiv((uint32_t)F));
        break;
    default: return PMENV_ERR_ARG;
    }
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

const char* pmenv_rollout_gather_env_path(int32_t N, int32_t F, int32_t W, int32_t S, int32_t aligned) {
    thread_local char text[160];
    text[0] = 0;
    if (N < 1 || F < 2 || W < 1 || S < 1 || aligned < 0 || aligned > 3) return text;
    replay_plan_describe(PMENV_REPLAY_ROLLOUT, replay_plan_rollout(N, F, W, S, aligned), text, sizeof(text), true);
    return text;
}

int pmenv_metrics(const double* returns, const double* values, const float* weights, int32_t T, int32_t B, int32_t N,
                  double risk_free_rate, double periods, double* out, hipStream_t stream) {
    if (!returns || !values || !weights || !out || T < 1 || B < 1 || N < 1 || !(periods > 0.0)) return PMENV_ERR_ARG;
    int rc = PMENV_OK;
    if (pmenv_tools::metrics(returns, values, weights, T, B, N, risk_free_rate, periods, out, stream, &rc)) return rc;
    // measured on MI355X (tools/bench_rows.py): the segment walk (the horizon split over
    // four waves per 64 envs) beside the turnover stream, in one launch — against the
    // thread-per-env walk and the two-launch form (profiles/rows_r01*/)
    const int tpe = N <= 256 ? N : 256, eb = 256 / tpe;
    const int nseg = (B + 63) / 64, nturn = (B + eb - 1) / eb;
    metrics_fused_kernel<<<(unsigned)(nseg + nturn), 256, 0, stream>>>(returns, values, weights, T, B, N,
                                                                       risk_free_rate, periods, tpe, eb, nseg,
                                                                       nturn, 1, out);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int pmenv_metrics_episodes(const double* returns, const double* values, const float* weights, const uint8_t* dones,
                           int32_t T, int32_t B, int32_t N, double init_value, double risk_free_rate, double periods,
                           int32_t max_episodes, double* out, int32_t* span, int32_t* count, hipStream_t stream) {
    if (!returns || !values || !weights || !dones || !out || !span || !count || T < 1 || B < 1 || N < 1 ||
        !(periods > 0.0) || max_episodes < 1)
        return PMENV_ERR_ARG;
    // pmenv_metrics' geometry: a segment-walk block per 64 envs, then the turnover blocks
    // (N <= 64: whole envs per wave, so eb is four times a wave's envs)
    const int tpe = N <= 256 ? N : 256, eb = N <= 64 ? 4 * (64 / N) : 256 / tpe;
    const int nseg = (B + 63) / 64, nturn = (B + eb - 1) / eb;
    metrics_env_fused_kernel<<<(unsigned)(nseg + nturn), 256, 0, stream>>>(
        returns, values, weights, dones, T, B, N, init_value, risk_free_rate, periods, max_episodes, tpe, eb, nseg,
        out, span, count);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

size_t pmenv_batch_reward_workspace(int32_t B) { return B < 1 ? 0 : batch_reward_work_doubles(B) * 8; }

// The batched reward's kernel choice for a [B, N] batch: the one decision the forward, the
// backward and pmenv_batch_reward_path all read.
//   N <= 64: a quad of lanes per row, EPL 8 (N <= 32) or 16 elements per lane, 64 rows per partial
//            record; at most 64 rows (the agents' BATCH_SIZE, config/pg.py:7): the whole forward
//            in one workgroup, one launch
//   N  > 64: a wave per row, EPL 2 / 4 / 8 elements per lane in registers up to N = 512, EPL 0
//            looping beyond; 16 rows per partial record
struct BatchRewardPlan {
    bool quad, small;
    int epl, parts;
};
static BatchRewardPlan batch_reward_plan(int32_t B, int32_t N) {
    BatchRewardPlan pl;
    pl.quad = N <= kQuadMaxN;
    pl.small = pl.quad && B <= kQuadRows;
    pl.epl = N <= 32 ? 8 : N <= kQuadMaxN ? 16 : N <= 128 ? 2 : N <= 256 ? 4 : N <= 512 ? 8 : 0;
    pl.parts = pl.quad ? (B + kQuadRows - 1) / kQuadRows : (int)batch_reward_blocks(B);
    return pl;
}

const char* pmenv_batch_reward_path(int32_t B, int32_t N) {
    thread_local char text[160];
    text[0] = 0;
    if (B < 1 || N < 1) return text;
    const BatchRewardPlan pl = batch_reward_plan(B, N);
    snprintf(text, sizeof(text), "%s<%d> | %s<%d> | parts=%d",
             pl.small ? "batch_reward_small_kernel" : pl.quad ? "batch_reward_rows_quad_kernel" : "batch_reward_rows_kernel",
             pl.epl, pl.quad ? "batch_reward_grad_quad_kernel" : "batch_reward_grad_kernel", pl.epl, pl.parts);
    return text;
}

int pmenv_batch_reward_forward(const float* a, const float* v_prev, const float* p, int32_t B, int32_t N,
                               int32_t reward_kind, int32_t norm, double scale, double* work,
                               float* reward_out, float* ret_out, hipStream_t stream) {
    if (!a || !v_prev || !p || !work || !reward_out || B < 1 || N < 1) return PMENV_ERR_ARG;
    if (reward_kind != PMENV_REWARD_LOG_RETURN && reward_kind != PMENV_REWARD_RETURN &&
        reward_kind != PMENV_REWARD_SHARPE)
        return PMENV_ERR_ARG;
    if (norm < PMENV_BNORM_GLOBAL_OR || norm > PMENV_BNORM_NONE) return PMENV_ERR_ARG;
    int rc = PMENV_OK;
    if (pmenv_tools::batch_reward_forward(a, v_prev, p, B, N, reward_kind, norm, scale, work, reward_out, ret_out,
                                          stream, &rc))
        return rc;
    const BatchRewardPlan pl = batch_reward_plan(B, N);
    // at most 64 rows (the agents' BATCH_SIZE, config/pg.py:7): one workgroup, one launch
    if (pl.small) {
        if (pl.epl == 8)
            batch_reward_small_kernel<8><<<1, kTrainBlock, 0, stream>>>(a, v_prev, p, B, N, reward_kind, norm, scale,
                                                                         work, reward_out, ret_out);
        else
            batch_reward_small_kernel<16><<<1, kTrainBlock, 0, stream>>>(a, v_prev, p, B, N, reward_kind, norm, scale,
                                                                          work, reward_out, ret_out);
        return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
    }
    // two launches: the row blocks' partials, then the final fold (a one-launch form with a
    // last-block ticket measured slower at every shape: DESIGN.md §7 f2)
    const int nparts = pl.parts;
    const unsigned g = (unsigned)nparts;
    if (pl.quad) {                // a quad of lanes per row
        if (pl.epl == 8)
            batch_reward_rows_quad_kernel<8><<<g, kTrainBlock, 0, stream>>>(a, v_prev, p, B, N, reward_kind, norm, work);
        else
            batch_reward_rows_quad_kernel<16><<<g, kTrainBlock, 0, stream>>>(a, v_prev, p, B, N, reward_kind, norm, work);
    } else {                      // wave per row, registers up to N = 512
        switch (pl.epl) {
        case 2: batch_reward_rows_kernel<2><<<g, kTrainBlock, 0, stream>>>(a, v_prev, p, B, N, reward_kind, norm, work); break;
        case 4: batch_reward_rows_kernel<4><<<g, kTrainBlock, 0, stream>>>(a, v_prev, p, B, N, reward_kind, norm, work); break;
        case 8: batch_reward_rows_kernel<8><<<g, kTrainBlock, 0, stream>>>(a, v_prev, p, B, N, reward_kind, norm, work); break;
        default: batch_reward_rows_kernel<0><<<g, kTrainBlock, 0, stream>>>(a, v_prev, p, B, N, reward_kind, norm, work);
        }
    }
    batch_reward_final_kernel<<<1, kTrainBlock, 0, stream>>>(B, reward_kind, norm, scale, work, reward_out, nparts);
    // the chosen per-row return, when asked for (the backward takes each row's choice itself)
    if (ret_out) batch_reward_select_kernel<<<(B + 255) / 256, 256, 0, stream>>>(B, norm, work, ret_out);
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

int pmenv_batch_reward_backward(const float* a, const float* v_prev, const float* p, int32_t B, int32_t N,
                                int32_t reward_kind, double scale, const double* work, const float* grad_out,
                                float* grad_a, hipStream_t stream) {
    if (!a || !v_prev || !p || !work || !grad_out || !grad_a || B < 1 || N < 1) return PMENV_ERR_ARG;
    const BatchRewardPlan pl = batch_reward_plan(B, N);
    const unsigned qgrid = (unsigned)pl.parts, wgrid = (unsigned)((B + 3) / 4);   // 64 rows | 4 rows per block
    if (pl.quad) {
        if (pl.epl == 8)
            batch_reward_grad_quad_kernel<8><<<qgrid, kTrainBlock, 0, stream>>>(a, v_prev, p, B, N, reward_kind, scale,
                                                                               work, grad_out, grad_a);
        else
            batch_reward_grad_quad_kernel<16><<<qgrid, kTrainBlock, 0, stream>>>(a, v_prev, p, B, N, reward_kind, scale,
                                                                                work, grad_out, grad_a);
    } else {
        switch (pl.epl) {
        case 2: batch_reward_grad_kernel<2><<<wgrid, 256, 0, stream>>>(a, v_prev, p, B, N, reward_kind, scale, work,
                                                                       grad_out, grad_a); break;
        case 4: batch_reward_grad_kernel<4><<<wgrid, 256, 0, stream>>>(a, v_prev, p, B, N, reward_kind, scale, work,
                                                                       grad_out, grad_a); break;
        case 8: batch_reward_grad_kernel<8><<<wgrid, 256, 0, stream>>>(a, v_prev, p, B, N, reward_kind, scale, work,
                                                                       grad_out, grad_a); break;
        default: batch_reward_grad_kernel<0><<<wgrid, 256, 0, stream>>>(a, v_prev, p, B, N, reward_kind, scale, work,
                                                                        grad_out, grad_a);
        }
    }
    return hipGetLastError() == hipSuccess ? PMENV_OK : PMENV_ERR_HIP;
}

}  // extern "C"

// ---------------------------------------------------------------- tools-build hooks
// The product library's hooks do nothing; tools/ab/pmenv_ab.hip (linked only into
// tools/libpmenv_ab.so) overrides these weak definitions.
namespace pmenv_tools {
__attribute__((weak, noinline)) void plan(pmenv*) {}
__attribute__((weak, noinline)) void release(pmenv*) {}
__attribute__((weak, noinline)) bool launch_scalar(const pmenv*, const StepParams&, hipStream_t) { return false; }
__attribute__((weak, noinline)) bool launch_advance(const pmenv*, const StepParams&, hipStream_t) { return false; }
__attribute__((weak, noinline)) bool launch_one(const pmenv*, const StepParams&, hipStream_t) { return false; }
__attribute__((weak, noinline)) bool launch_small(const pmenv*, const StepParams&, hipStream_t) { return false; }
__attribute__((weak, noinline)) bool launch_gen(const pmenv*, const StepParams&, hipStream_t) { return false; }
__attribute__((weak, noinline)) bool launch_fused(const pmenv*, const StepParams&, int, uint32_t, hipStream_t) {
    return false;
}
__attribute__((weak, noinline)) bool launch_relay(const pmenv*, const StepParams&, const RelayParams&, unsigned,
                                                  hipStream_t) {
    return false;
}
__attribute__((weak, noinline)) bool launch_flat1(const pmenv*, const StepParams&, unsigned, bool, int,
                                                  hipStream_t) {
    return false;
}
__attribute__((weak, noinline)) bool gae(const float*, const float*, const uint8_t*, float*, float*, int32_t,
                                         int32_t, float, float, hipStream_t, int*) {
    return false;
}
__attribute__((weak, noinline)) bool replay_gather(const float*, int32_t, int32_t, int32_t, int32_t, const int32_t*,
                                                   const float*, const float*, int32_t, int32_t, const int32_t*,
                                                   const int32_t*, int32_t, float*, float*, float*, float*,
                                                   hipStream_t, int*) {
    return false;
}
__attribute__((weak, noinline)) void replay_seq_knobs(int*, int*) {}
__attribute__((weak, noinline)) int ind_form() { return -1; }
__attribute__((weak, noinline)) bool rollout_gather(const float*, int32_t, int32_t, int32_t, int32_t, const int32_t*,
                                                    const float*, int32_t, int32_t, int32_t, const int32_t*,
                                                    const int32_t*, int32_t, float*, hipStream_t, int*) {
    return false;
}
__attribute__((weak, noinline)) bool metrics(const double*, const double*, const float*, int32_t, int32_t, int32_t,
                                             double, double, double*, hipStream_t, int*) {
    return false;
}
__attribute__((weak, noinline)) bool batch_reward_forward(const float*, const float*, const float*, int32_t, int32_t,
                                                          int32_t, int32_t, double, double*, float*, float*,
                                                          hipStream_t, int*) {
    return false;
}
}  // namespace pmenv_tools
