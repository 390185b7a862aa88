/*
 * pmenv.h — C ABI of the MI355X-native vectorised portfolio environment.
 *
 * This is the drop-in boundary for the hot path of zachramsey/pm-rl:
 *   env/sim/trading_env.py   (TradingEnv.__init__ :8-18, reset :21-41, step :44-105)
 *   env/sim/weight_buffer.py (ActionBuffer :5-51 — the W x N weight ring)
 *   env/reward.py            (Reward :6-31 — returns / log_returns / sharpe_ratio)
 *   data/instrument.py:79    (price relatives y_t = close_t / close_{t-1})
 *   data/instrument.py:339-356 (sliding window; fused here as an in-place window advance)
 *
 * The reference is a single-env Python class driven from train/on_policy.py:59-67;
 * here B lockstep envs share one handle and one HIP kernel launch per step.
 *
 * Conventions
 *   - every entry point returns 0 (PMENV_OK) or a negative pmenv_status;
 *     pmenv_last_error(h) then holds a message.
 *   - every data pointer passed to reset/step is a DEVICE pointer owned by the
 *     caller (e.g. a torch tensor's data_ptr()); env state is owned by the handle.
 *   - layouts are dense row-major: obs [B, N, W, F] fp32, action [B, N] fp32,
 *     prices [B, N] fp32, bar [B, N, F-1] fp32, reward [B] fp32.
 *   - one handle belongs to one device; calls on a handle are not thread-safe;
 *     reset/step enqueue on `stream` and never synchronise the host, allocate,
 *     or free (they are hipGraph-capturable).
 */
#ifndef PMENV_H
#define PMENV_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: pmenv_window_written / pmenv_state_written and PMENV_STEP_PATH_RELAY added;
 *    pmenv_cfg_default's ret_mode is PMENV_RET_GROSS (trading_env.py:88 for every reward
 *    kind; was AUTO in 1) */
/* 3: pmenv_step_host / pmenv_reset_host (host buffers, the reference driver's call shape) */
/* 4: pmenv_replay_gather_nstep (n-step return samples of the replay ring) */
/*    (pmenv_replay_gather_seq, sequence samples of the same ring, was added under 4: a new
 *    symbol breaks no caller; pmenv's loader names a symbol that a stale library lacks;
 *    pmenv_gae_path, the GAE pass's kernel by name, likewise; pmenv_restart_days, per-env
 *    episodes on the resident series, likewise; pmenv_replay_path, the sample gathers'
 *    kernel by name, likewise; pmenv_replay_valid_build, pmenv_replay_valid_select,
 *    pmenv_replay_gather_nstep_env, pmenv_replay_gather_seq_env and pmenv_prio_fill_env, the
 *    replay of envs that end their episodes on their own, likewise; pmenv_rollout_gather_env and
 *    pmenv_rollout_gather_env_path, the compact rollout of such envs, likewise;
 *    pmenv_metrics_episodes, the trajectory metrics of such envs per episode, likewise;
 *    pmenv_step_path_for, the step's kernels and geometry for a cfg without a device, likewise;
 *    pmenv_batch_reward_path, the batched reward's kernels by name, likewise;
 *    pmenv_ffd_weights, pmenv_ffd_apply, pmenv_ffd_path, pmenv_scale_workspace, pmenv_scale_fit
 *    and pmenv_scale_apply, the loader's feature stages on the device, likewise;
 *    pmenv_ind_layout, pmenv_ind_workspace, pmenv_ind_apply and pmenv_ind_path, the loader's
 *    technical indicators on the device, likewise; pmenv_ffd_table, pmenv_adf,
 *    pmenv_adf_workspace, pmenv_adf_path, pmenv_adf_maxlag, pmenv_adf_pvalue and
 *    pmenv_adf_search_update, the search for the orders of differencing, likewise) */
#define PMENV_ABI_VERSION 4

/* Opaque HIP stream (identical to HIP's own typedef); NULL = default stream. */
typedef struct ihipStream_t* hipStream_t;

typedef struct pmenv pmenv; /* opaque handle */

typedef enum pmenv_status {
    PMENV_OK = 0,
    PMENV_ERR_ARG = -1,    /* bad config value or NULL where a pointer is required */
    PMENV_ERR_SHAPE = -2,  /* shape mismatch; weight_buffer.py:18-19 raises ValueError */
    PMENV_ERR_HIP = -3,    /* a HIP runtime call failed */
    PMENV_ERR_ALIGN = -4   /* pointer not 4-byte aligned */
} pmenv_status;

/* Reward kinds. The reference step() hard-codes log_returns (trading_env.py:99);
 * REWARD switch at trading_env.py:93-98 is commented out; env/reward.py:15-31
 * restates returns/log_returns/sharpe_ratio; differential Sharpe is absent from
 * the reference (north star addition, parity unpinned by the reference). */
typedef enum pmenv_reward_kind {
    PMENV_REWARD_LOG_RETURN = 0,  /* r = log(ret) * scale           trading_env.py:99 */
    PMENV_REWARD_RETURN = 1,      /* r = ret * scale                reward.py:20-21   */
    PMENV_REWARD_SHARPE = 2,      /* (mean(ret_1..t) - rf) / std(ret_1..t, ddof=1) * scale, reward.py:26-31 (NaN while t < 2, as numpy) */
    PMENV_REWARD_DIFF_SHARPE = 3  /* Moody-Saffell differential Sharpe on R = ret - 1, EMA rate eta */
} pmenv_reward_kind;

/* Action normalisation predicate (trading_env.py:58 vs agent/pg/pg.py:52). */
typedef enum pmenv_norm_mode {
    PMENV_NORM_AND = 0, /* reference env: normalise iff !isclose(sum,1) AND min<0; exp(w)/sum(exp(w)) */
    PMENV_NORM_OR = 1   /* batched trainer: normalise iff !isclose(sum,1) OR min<0; softmax */
} pmenv_norm_mode;

/* Weight-history channel order once the ring has wrapped (weight_buffer.py:38-44). */
typedef enum pmenv_ring_mode {
    PMENV_RING_STORAGE = 0, /* reference: ring returned in storage order after wrap */
    PMENV_RING_CHRONO = 1   /* intended: oldest..newest always */
} pmenv_ring_mode;

/* Which value the return uses (trading_env.py:75,88). The reference has two answers:
 * step() takes log(value / (mu * V_prev)) (trading_env.py:75,88,99 — the commission is
 * excluded) and records that ratio as info["returns"] (:90), while env/reward.py:20-31
 * forms returns / log_returns / sharpe_ratio from info["values"], i.e. V_t / V_{t-1}
 * (trading_env.py:80 — commission included). GROSS, the default, is step()'s answer for
 * every reward kind, so info["returns"] and every reward match trading_env.py whatever
 * the commission. NET and AUTO are opt-in; with commission 0 all three agree. */
typedef enum pmenv_ret_mode {
    PMENV_RET_GROSS = 0, /* ret = value / (mu * V_prev): excludes commission (trading_env.py:88) — default */
    PMENV_RET_NET = 1,   /* ret = value / V_prev: includes commission (reward.py:20-31 over info["values"]) */
    PMENV_RET_AUTO = 2   /* opt-in: GROSS for PMENV_REWARD_LOG_RETURN (step()'s hard-coded reward,
                            trading_env.py:99), NET for the kinds only reward.py defines (returns,
                            sharpe_ratio) and for diff_sharpe (resolved at create) */
} pmenv_ret_mode;

typedef struct pmenv_cfg {
    int32_t num_envs;       /* B */
    int32_t num_assets;     /* N  (config/base.py:29 NUM_ASSETS) — asset 0 is cash */
    int32_t window;         /* W  (config/base.py:28 WINDOW_SIZE) */
    int32_t features;       /* F  (last channel F-1 carries the weight history, trading_env.py:103) */
    int32_t close_channel;  /* channel of the close price in obs / bar (price relatives) */
    int32_t reward_kind;    /* pmenv_reward_kind */
    int32_t norm_mode;      /* pmenv_norm_mode */
    int32_t ring_mode;      /* pmenv_ring_mode */
    int32_t ret_mode;       /* pmenv_ret_mode, default GROSS (AUTO is resolved at create; pmenv_get_cfg returns the result) */
    int32_t mu_max_iter;    /* cap on the commission fixed point (trading_env.py:70 has none) */
    double init_cash;       /* config/base.py:47 INITIAL_CASH = 25000 */
    double commission;      /* config/base.py:48 COMISSION = 0.0 */
    double reward_scale;    /* config/base.py:52 REWARD_SCALE = 1 */
    double risk_free_rate;  /* config/base.py:53 RISK_FREE_RATE = 0.04 (sharpe_ratio only) */
    double sharpe_eta;      /* EMA rate of the differential Sharpe reward */
    double mu_tol;          /* fixed-point tolerance, trading_env.py:70 uses 1e-10 */
} pmenv_cfg;

/* Fills cfg with the reference defaults for the given shapes
 * (close_channel = 3 for [open, high, low, close, weight] when F >= 5, else 0). */
void pmenv_cfg_default(pmenv_cfg* cfg, int32_t num_envs, int32_t num_assets,
                       int32_t window, int32_t features);

int32_t pmenv_abi_version(void);

/* Allocates per-env state on `device` (value f64, update counter, W x N weight
 * ring, reward-statistic pair) and puts every env in the reset state.
 * Replaces TradingEnv.__init__ (trading_env.py:8-18) + ActionBuffer.__init__ (weight_buffer.py:6-11). */
int pmenv_create(const pmenv_cfg* cfg, int device, pmenv** out);
/* Same, with the state living in caller-provided device memory of at least
 * pmenv_state_bytes_for(cfg) bytes, 16-B aligned (e.g. a torch uint8 tensor, so
 * the host wrapper gets zero-copy views); the handle never frees it. */
size_t pmenv_state_bytes_for(const pmenv_cfg* cfg);
int pmenv_create_in(const pmenv_cfg* cfg, int device, void* state, size_t state_bytes, pmenv** out);
/* Byte offsets of the state fields inside the state blob:
 * [0] value f64[B], [1] stat_a f64[B], [2] stat_b f64[B], [3] counter i32[B],
 * [4] ring f32[B,W,N], [5] nonfinite u64, [6] last_close f32[B,N] (the close of
 * the window's last day, i.e. obs[b, n, W-1, close_channel], kept by reset/step
 * so the advance path never re-reads the window to form price relatives),
 * [7] w_new f32[B,N] (post-drift weights of the latest step = the ring slot just
 * written, stored densely for the streaming kernel). */
#define PMENV_STATE_FIELDS 8
int pmenv_state_layout(const pmenv_cfg* cfg, size_t offsets[PMENV_STATE_FIELDS]);
int pmenv_destroy(pmenv* h);
const char* pmenv_last_error(const pmenv* h);
int pmenv_get_cfg(const pmenv* h, pmenv_cfg* out);

/* TradingEnv.reset (trading_env.py:21-41): value <- init_cash, ring <- e0, and
 * obs[:, :, :, F-1] <- get_all() (weight_buffer.py:32-44) in place.
 * mask [B] (uint8, device) selects which envs reset; NULL resets all.
 * obs may be NULL (state-only reset). */
int pmenv_reset(pmenv* h, float* obs, const uint8_t* mask, hipStream_t stream);

/* Per-env episodes on a resident series (pmenv_step_args.day): call after every such step.
 * day, end, restart, done: device arrays of B elements; series [series_days, N, F-1], the
 * one the steps read; obs the window the preceding step left (in place, or its obs_out).
 * On entry day[b] is the bar that step appended. With next = day[b] + 1:
 *   next <  end[b]: day[b] = next, done[b] = 0; nothing else of env b is read or written.
 *   next >= end[b]: done[b] = 1 and env b restarts: obs[b, n, t, f] = series[restart[b] + t, n, f]
 *     for f < F-1 (days outside the series: NaN, as pmenv_window_init_days), channel F-1 and
 *     the state (value, counter, statistics, ring, w', last closes) as pmenv_window_init_days
 *     followed by pmenv_reset(obs, mask) leave them, and day[b] = restart[b] + W, the next
 *     bar to append. The non-finite counter is not touched.
 * end[b] is one past the last bar env b may append; the caller keeps end[b] <= series_days
 * and restart[b] + W < end[b] (not checked on the device). One launch whose work is
 * proportional to the envs that restart; enqueues on `stream`, never synchronises, allocates
 * or frees, hipGraph-capturable. Like pmenv_reset it leaves the flat and relay steps' copies
 * stale on every call (they re-prime on the next step). NULL obs, series, day, end, restart
 * or done: PMENV_ERR_ARG. */
int pmenv_restart_days(pmenv* h, float* obs, const float* series, int32_t series_days,
                       int32_t* day, const int32_t* end, const int32_t* restart,
                       uint8_t* done, hipStream_t stream);

/* Optional per-step outputs (the reference's info dict, trading_env.py:80,85,90,100). */
typedef struct pmenv_step_args {
    const float* action;   /* [B, N]  target weights (raw policy output)            */
    const float* prices;   /* [B, N]  price relatives y_t, or NULL (needs bar)       */
    const float* bar;      /* [B, N, F-1] new day's market channels, or NULL; with `day`
                              set: a market series [series_days, N, F-1] shared by all envs */
    const int32_t* day;    /* NULL, or [B] device day index: env b's bar is bar[day[b]]
                              (resident-series data path; a day outside
                              [0, series_days) reads NaN and is counted non-finite)   */
    int32_t series_days;
    float* obs;            /* [B, N, W, F] in/out                                     */
    float* obs_out;        /* advance mode only: NULL = advance obs in place; else the
                              advanced window is written here and obs is left untouched
                              (double-buffered windows; must not overlap obs)           */
    float* reward;         /* [B] out, may be NULL                                    */
    double* ret;           /* [B] out (info["returns"]), may be NULL                  */
    float* weights;        /* [B, N] out post-drift weights (info["actions"]), may be NULL */
    uint32_t phases;       /* 0 = whole step; PMENV_PHASE_SCALAR / PMENV_PHASE_ADVANCE run
                              one launch of the two-launch advance path (the advance
                              phase must follow the scalar phase of the same step;
                              used to time the streaming kernel on its own). Where the
                              step is one launch (step_flat_kernel, step_env_kernel,
                              step_relay_kernel, the per-env surface step) the scalar
                              phase runs all of it, the advance phase nothing; the
                              surface step past the Infinity Cache is two launches (the
                              scalar step, then surface_stream_kernel rewriting channel
                              F-1), so its scalar phase alone leaves that channel stale */
} pmenv_step_args;

#define PMENV_PHASE_SCALAR 1u
#define PMENV_PHASE_ADVANCE 2u

/* TradingEnv.step (trading_env.py:44-105) for all B envs in one kernel.
 *  - bar == NULL  ("surface" mode, the reference's own contract): obs is the
 *    caller's next-day window; only channel F-1 is rewritten from the ring.
 *    prices must be given.
 *  - bar != NULL  ("advance" mode, the north-star fused path): obs is the
 *    env-owned window returned by the previous reset/step; it is advanced one
 *    day in place (instrument.py:339-356 sliding window), the bar is appended
 *    at t = W-1, and if prices == NULL the relatives are
 *    bar[close] / obs[W-1, close] (instrument.py:79), with obs[W-1, close]
 *    taken from the env's last_close state (equal to it by construction).
 *    The window's channel F-1 is the ring itself here: the step shifts it with
 *    the window (or, storage order with the ring full, rewrites only the slot),
 *    so an edit the caller makes to that channel persists, where surface mode
 *    rewrites the whole channel from the ring; market-channel edits are honoured
 *    in both modes (announce in-place edits with pmenv_window_written).
 * Portfolio value (f64, env-owned) is readable through pmenv_value(). */
int pmenv_step_ex(pmenv* h, const pmenv_step_args* args, hipStream_t stream);
int pmenv_step(pmenv* h, const float* action, const float* prices, const float* bar,
               float* obs, float* reward, hipStream_t stream);

/* TradingEnv.step / reset with HOST buffers — the call shape of the reference's own driver,
 * which hands the env the data loader's CPU tensors (train/on_policy.py:59-67, :81-89;
 * trading_env.py:21-41, :44-105). Surface contract only: action [B, N], prices [B, N] and
 * the caller's window obs [B, N, W, F] are host memory (pageable is fine); channel F-1 of
 * obs is rewritten in place, exactly as trading_env.py:32 / :103 do. Outputs, each
 * optional (NULL): reward [B] f32, value [B] f64 (TradingEnv.value after the call), ret [B]
 * f64 (info["returns"]), weights [B, N] f32 (info["actions"]).
 * The step kernel reads the action, the prices and the window's last closes (N floats per
 * env) straight from pinned, device-mapped staging, and writes the [N, W] weight channel
 * and the outputs back into it; the market channels never cross PCIe. SYNCHRONOUS: the
 * outputs are in place when the call returns (so not graph-capturable: PMENV_ERR_ARG under
 * capture). Up to 8 envs, and when this handle has enqueued no device work since its last
 * host-buffer call, pmenv_step_host runs in one resident workgroup that polls the staging (no
 * launch per call; it exits after 20 ms without a call or at pmenv_destroy); otherwise it is
 * one launch on `stream`, ordered after the handle's earlier work there. Other kernels that
 * read or write this handle's state must be complete before a host-buffer call. The staging is
 * allocated on the first call. The host side (the last closes gathered, the channel scattered
 * into obs) is serial on the calling thread: B*N*W strided stores per call. */
int pmenv_step_host(pmenv* h, const float* action, const float* prices, float* obs, float* reward, double* value,
                    double* ret, float* weights, hipStream_t stream);
int pmenv_reset_host(pmenv* h, float* obs, double* value, hipStream_t stream);

/* Which kernels the advance path launches for this handle's shape (diagnostics):
 * "<obs_out path> (obs_out) | <in-place path> (in place)", each either
 * "step_flat_kernel" (the whole step in one launch over 16 KiB window tiles),
 * "step_flat_vec_kernel" (the same for 64 < N <= 512),
 * "step_env_kernel" (the whole step in one launch, one workgroup per env) or
 * "<scalar step>+<window stream>"
 * (two launches; for F != 5 the stream is advance_gen_kernel); or, for F != 5 or windows that
 * are not 16-B granular, "step_tiny_kernel" (one workgroup per env, the window staged in LDS:
 * env windows of at most 2,048 floats, N <= 64), "step_small_kernel" (one workgroup per env,
 * the window in registers: env windows of at most 16,384 floats) or "step_advance_lds_kernel" (the LDS-tiled
 * fallback, any F).
 * The choice is the handle's shape plan: a pure function of its cfg and of
 * pmenv_set_step_path, made by one host-only header (csrc/step_plan.h) that pmenv_create,
 * pmenv_set_step_path, pmenv_step_ex's dispatch and this string all go through. */
const char* pmenv_step_path(const pmenv* h);
/* The same plan without a device or a handle: exactly what pmenv_step_path returns for a
 * fresh handle of `cfg` after pmenv_set_step_path(path) (a pmenv_step_path_kind; the
 * "device-sequenced" notes belong to a handle's history and never appear here). With
 * detail != 0 the plan's geometry follows after " -- " as space-separated key=value fields
 * in a fixed order, each printed whether or not the shape takes that form:
 *   flat1=BxV (step_flat_kernel's threads x 16-B chunks per thread), relay=BxV:KL/KA
 *   (step_relay_kernel's tiles and its scalar step's lanes per env / strided assets per lane),
 *   stream_ip=BxV (the in-place flat stream), pol=DB/IP (the streams' cache policy, 1 = nt),
 *   gen=BxV (advance_gen_kernel), k1= reg | lds | LxA | LxAs (the scalar step's form),
 *   one_waves (step_env_kernel's waves per workgroup), small=BxE (step_small_kernel), tiny,
 *   surf_stream (surface steps as scalar step + surface_stream_kernel), rows_per_tile and vec
 *   (the LDS fallback).
 * Returns "" for a cfg pmenv_create rejects, a path the shape does not fit, or NULL. The
 * string lives in thread-local storage until the thread's next call. */
const char* pmenv_step_path_for(const pmenv_cfg* cfg, int32_t path, int32_t detail);

/* Advance-mode step implementation. AUTO (the default) picks per shape and window
 * mode; ONE_LAUNCH forces step_env_kernel (one workgroup per env: F = 5, W >= 2,
 * N <= 64, the env window within 64 KiB of LDS); TWO_LAUNCH forces the scalar-step
 * kernel followed by the window stream (F = 5, 16-B granular env windows; or the generic
 * stream advance_gen_kernel for 2 <= F <= 16, F != 5, 16-B granular env windows with
 * W F >= 17, which AUTO also takes for such windows above 2 MiB in both modes, 16 MiB
 * where the env window is at most 2,048 floats with N <= 64); FLAT forces
 * step_flat_kernel (the whole step in one launch over fixed 16 KiB tiles of the window:
 * F = 5, W >= 2, env windows of >= 148 16-B chunks, N <= 64 — or, as step_flat_vec_kernel,
 * 64 < N <= 512 with W >= 14). Returns PMENV_ERR_ARG
 * (handle unchanged) when the shape does not fit the requested path. For N <= 64 every
 * path gives the same bits; the N > 64 scalar-step forms reduce in another order.
 *
 * FLAT keeps a per-step snapshot of the state its scalar step reads and, in place, the
 * halo of its tiles, both produced by the previous step: a caller that writes the state
 * blob (pmenv_create_in, e.g. the value) or an in-place window outside this API — or that
 * hands in a different window at the address of the last one — must say so before the
 * next step: pmenv_state_written / pmenv_window_written (pmenv_set_state and pmenv_reset
 * do it themselves; so does every other step path). The reference keeps no copy of the
 * caller's features (trading_env.py:102-105), so every such edit is honoured.
 * From the first FLAT step, reset or invalidation enqueued while `stream` is being captured
 * into a hipGraph on, the handle sequences its FLAT steps on the device (a small
 * flat_seq_kernel before each step_flat_kernel reads the parity and the snapshot's
 * validity from device memory, so graph replays and eager calls interleave freely;
 * pmenv_step_path then says "device-sequenced").
 *
 * RELAY forces step_relay_kernel: the two-launch path's scalar step and window stream in
 * ONE launch — scalar workgroups (one run per env) relay w' and the counter to the stream
 * tiles through epoch-tagged words in handle memory (F = 5, W >= 2, 16-B granular env
 * windows, N <= 512; the same bits as TWO_LAUNCH). In place it keeps the tiles' halo from
 * the previous step, under the same pmenv_window_written rule as FLAT. From the first call of
 * a handle enqueued while a stream is being captured into a hipGraph on, its relay steps are
 * device-sequenced (a small relay_prime_kernel before each step_relay_kernel reads the epoch,
 * the parity and the copies' validity from device memory), so captured and eager relay steps
 * interleave freely; pmenv_step_path then says "relay steps device-sequenced".
 * No dispatch-order assumption: a tile polls its rows' relay words a bounded number of times
 * and, if one is still missing (its scalar block not yet dispatched), defers — it stores
 * nothing, lists itself for the step and exits; the scalar blocks run the listed tiles once
 * their words have arrived (one run per tile, under a claim word). In blockIdx dispatch order
 * no tile defers; with every tile dispatched before every scalar block the step completes with
 * the same bits. (pmenv_gae_ex's look-back pass likewise: a wave that waits too
 * long computes the map itself.) */
typedef enum pmenv_step_path_kind {
    PMENV_STEP_PATH_AUTO = 0,
    PMENV_STEP_PATH_ONE_LAUNCH = 1,
    PMENV_STEP_PATH_TWO_LAUNCH = 2,
    PMENV_STEP_PATH_FLAT = 3,
    PMENV_STEP_PATH_RELAY = 4
} pmenv_step_path_kind;
int pmenv_set_step_path(pmenv* h, int32_t path);

/* The caller wrote the in-place window `obs` between steps (features it owns and may
 * edit, trading_env.py:102-105), or hands in a new window at a previous one's address:
 * the next FLAT step re-reads the tile halo from the window (enqueued on `stream`; a
 * no-op for the other step paths, which keep nothing of the window). */
int pmenv_window_written(pmenv* h, const float* obs, hipStream_t stream);
/* The caller wrote the state blob (pmenv_value, pmenv_counter, pmenv_ring or any field of
 * pmenv_state_layout) outside pmenv_set_state: the next FLAT step re-primes its snapshot
 * from the state (and its halo from the window). */
int pmenv_state_written(pmenv* h, hipStream_t stream);

/* Device pointer to the env-owned portfolio values [B] f64 (TradingEnv.value). */
double* pmenv_value(pmenv* h);
/* Device pointer to the weight ring [B, W, N] f32 (ActionBuffer.buffer) and
 * update counters [B] i32 (ActionBuffer.idx = (1 + k) % W, is_full = k >= W-1). */
float* pmenv_ring(pmenv* h);
int32_t* pmenv_counter(pmenv* h);

/* Checkpoint: the whole env state as one opaque device blob. */
size_t pmenv_state_bytes(const pmenv* h);
int pmenv_get_state(pmenv* h, void* dst_device, hipStream_t stream);
int pmenv_set_state(pmenv* h, const void* src_device, hipStream_t stream);

/* Count of envs whose reward or value came out non-finite since create
 * (synchronises `stream`). */
int pmenv_nonfinite_count(pmenv* h, uint64_t* out, hipStream_t stream);

/* ---- synthetic data path (Philox4x32-10, key = seed) ---- */

/* OHLC random walk: series [T, B, Fm=4 ... ] written as [T][B][N][4] =
 * [open, high, low, close]; env ids are env_offset .. env_offset+B-1 so a
 * sharded run generates exactly the slice of the unsharded series. */
int pmenv_synth_series(float* series, int32_t T, int32_t B, int32_t N,
                       int64_t env_offset, uint64_t seed, float sigma, hipStream_t stream);
/* Softmax-of-N(0,1) simplex actions [T][B][N]. */
int pmenv_synth_actions(float* actions, int32_t T, int32_t B, int32_t N,
                        int64_t env_offset, uint64_t seed, hipStream_t stream);
/* obs[b, n, t, f] = series[t, b, n, f] for t < W, f < 4; channel F-1 left for reset. F must be 5. */
int pmenv_window_init(float* obs, const float* series, int32_t B, int32_t N,
                      int32_t W, int32_t F, hipStream_t stream);
/* Resident market series (data/instrument.py:339-356 windows over one shared series):
 * obs[b, n, t, f] = series[start[b] + t, n, f] for t < W, f < F-1 (channel F-1 = 0,
 * written by reset). series [T, N, F-1]; start [B] device int32 with
 * 0 <= start[b] <= T - W (envs outside get NaN windows). */
int pmenv_window_init_days(float* obs, const float* series, int32_t T, int32_t N, int32_t F,
                           const int32_t* start, int32_t B, int32_t W, hipStream_t stream);

/* ---- rollout returns (north star: replay/rollout_buffer.py's GAE / discounted
 * return pass as a device scan; the reference stores (s,a,v,r) but computes no
 * returns, rollout_buffer.py:43-57) ---- */

/* adv[t,b] = delta_t + gamma*lambda*(1-done[t,b])*adv[t+1,b],
 * delta_t = r[t,b] + gamma*(1-done[t,b])*v[t+1,b] - v[t,b];  ret = adv + v.
 * rewards/dones [T,B], values [T+1,B]; dones may be NULL. */
int pmenv_gae(const float* rewards, const float* values, const uint8_t* dones,
              float* adv, float* ret, int32_t T, int32_t B, float gamma, float lam,
              hipStream_t stream);
/* The same pass with caller-owned device scratch of pmenv_gae_workspace(T, B) bytes
 * (0 when the shape does not use it): rollouts with few envs (B < 8192) and long
 * horizons (T >= 512) also split the horizon across workgroups in ONE launch — each
 * chunk publishes its affine map and an epoch-tagged flag in `work`, then composes the
 * later chunks' maps (replaces round 3's two launches). `work` must be 8-B aligned; it
 * may be reused by later calls (each call tags its flags with a fresh epoch) but not
 * shared by two calls in flight. work == NULL, too small or misaligned: as pmenv_gae.
 * Enqueued while `stream` is being captured into a hipGraph: as pmenv_gae too, and `work`
 * is left untouched — the look-back's epoch is chosen by the host at enqueue time, so a
 * replayed call would find its own epoch already in the flags and could compose the
 * previous replay's maps; the tile, scan and loop kernels keep no state between calls. */
size_t pmenv_gae_workspace(int32_t T, int32_t B);
int pmenv_gae_ex(const float* rewards, const float* values, const uint8_t* dones,
                 float* adv, float* ret, int32_t T, int32_t B, float gamma, float lam,
                 double* work, size_t work_bytes, hipStream_t stream);
/* The kernel instantiation a [T, B] call takes outside stream capture, as a static string
 * ("gae_tile_kernel<8,16,1,2>", "gae_tile_kernel<8,8>", "gae_tile_kernel<8,8,8,2>",
 * "gae_scan_kernel", "gae_kernel", "gae_lookback_kernel<8,8>", "gae_lookback_kernel<8,16>";
 * "" for T < 1 or B < 1). pmenv_gae: work_bytes = 0. pmenv_gae_ex: the call's work_bytes
 * and work_aligned = (work != NULL and 8-B aligned). Host only: launches nothing. */
const char* pmenv_gae_path(int32_t T, int32_t B, size_t work_bytes, int work_aligned);

/* Per-rank advantage moments {count, sum, sum of squares} in f64 into out[3]
 * (the only cross-GPU exchange: a 24-byte all-reduce over xGMI). `work` is
 * caller-owned device scratch of pmenv_moments_workspace() bytes (per-block
 * partials; two calls in flight need two workspaces). Deterministic. */
size_t pmenv_moments_workspace(void);
int pmenv_moments(const float* x, int64_t n, double* out, double* work, hipStream_t stream);

/* ---- the loader's feature stages on the device (data/ffd.py, data/instrument.py:257-336):
 * fixed-width-window fractional differencing and the per-column scalers over x [T, C] f32,
 * the C = N * (F-1) columns contiguous (the [T, N, F-1] bar layout). ---- */

/* data/ffd.py:38-47 as the reference's CPU path computes it: the taps of order d over a
 * series of T rows, w_0 = 1, w_k = f32(prod_{i <= k} p_i), p_k = (-(d+1)) / k + 1 in f32, the
 * running product in f64 and every tap rounded to f32; *width = max{k < T : |w_k| > thres}
 * (:43) and the filter is taps 0 .. width-1 (:47 drops tap `width` itself: d = 1 gives the
 * single tap [1], the identity). d = 0: "leave the column alone", width 0 (:84). Writes
 * min(*width, cap) taps; taps may be NULL with cap = 0 (the width only). Host only.
 * PMENV_ERR_ARG: T < 2, d or thres negative or not finite, NULL width. */
int pmenv_ffd_weights(double d, double thres, int32_t T, float* taps, int32_t cap, int32_t* width);
/* data/ffd.py:80-89 (one conv1d per column, clipped by the widest filter) in one launch:
 * out[r, c] = sum_{j < width[c]} taps[j, c] * x[max_width + r - j, c] for r < T - max_width.
 * taps [max_width, C] f32 (tap-major; rows >= width[c] of a column are not read), width [C]
 * int32 on the device (clamped to [0, max_width]), out [T - max_width, C] f32. Each output is
 * one f64 chain in ascending j, acc = fma((double)w_j, (double)x[t-j], acc) from 0, rounded
 * once to f32: the product of two f32 values is exact in f64, so the bits depend on no
 * geometry. A column of width 0 copies x[max_width + r]. A NaN in x makes exactly the
 * width[c] outputs of its column that read it NaN. out must overlap neither x nor taps
 * (PMENV_ERR_ARG); max_width >= T, T < 1, C < 1: PMENV_ERR_ARG. 4-B alignment. No allocation,
 * no synchronisation, capturable. */
int pmenv_ffd_apply(const float* x, int32_t T, int32_t C, const float* taps, const int32_t* width,
                    int32_t max_width, float* out, hipStream_t stream);
/* The kernel pmenv_ffd_apply launches for a shape and its geometry, e.g.
 *   "ffd_apply_kernel<8,8> cw=64 slots=1 rows=32 grid=345x4 block=256"
 * <outputs per lane, taps per block>, cw columns and slots time slots per wave, rows output
 * rows per workgroup, grid = time chunks x column groups. "" for a refused shape. Host only;
 * the string is thread-local and valid until the thread's next call. */
const char* pmenv_ffd_path(int32_t T, int32_t C, int32_t max_width);

/* data/instrument.py:318-336 (sklearn's MinMaxScaler / StandardScaler fitted per (ticker,
 * feature) column, config/base.py:25). */
typedef enum pmenv_scale_method {
    PMENV_SCALE_MINMAX = 0,   /* stats = {min, max};  y = (x - min) / (max - min) */
    PMENV_SCALE_STANDARD = 1  /* stats = {mean, std} (ddof 0); y = (x - mean) / std */
} pmenv_scale_method;
/* Device scratch of a [T, C] fit in bytes (two doubles per 256-row chunk and column; two
 * fits in flight need two workspaces). 0 for a refused shape. */
size_t pmenv_scale_workspace(int32_t T, int32_t C);
/* stats [2, C] f64 on the device from x [T, C]; NaNs are skipped as sklearn's nanmin /
 * nanmax / nanmean do (a column without a number: NaN stats). The standard fit takes two
 * passes in f64, the mean and then the squares about it. Deterministic; stats and work 8-B
 * aligned. No allocation, no synchronisation, capturable. */
int pmenv_scale_fit(const float* x, int32_t T, int32_t C, int32_t method, double* stats, double* work,
                    size_t work_bytes, hipStream_t stream);
/* y[t, c] = f32(((double)x[t, c] - stats[0, c]) / den), den = max - min or std, 1 where that
 * is 0 (sklearn's zero-scale rule); a NaN passes through. stats may come from any fit (test
 * rows scaled with train statistics); y may be x. */
int pmenv_scale_apply(const float* x, int32_t T, int32_t C, int32_t method, const double* stats, float* y,
                      hipStream_t stream);

/* ---- the loader's technical indicators on the device (data/instrument.py:207-232 runs TA-Lib
 * once per ticker over the f64 OHLCV columns and appends every output as an f32 channel;
 * config/base.py:30-44 names the eleven below). bars [T, N, C] f32; every element is widened
 * to f64 on load, all arithmetic is f64, every output is rounded once to f32. The definitions
 * are this header's (DESIGN.md "Technical indicators" has the table): TA-Lib's default
 * algorithms restated — SMA-seeded EMA, Wilder smoothing, unstable period 0, SMA smoothing
 * only — with one deliberate deviation: dx is 0 where its true-range sum or DI- + DI+ is
 * within 1e-8 of zero (TA-Lib repeats its previous output). ---- */
typedef enum pmenv_ind_kind {
    PMENV_IND_EMA = 0,     /* p = {timeperiod};                       1 output,  L = p-1 */
    PMENV_IND_BBANDS = 1,  /* p = {timeperiod}, f = {nbdevup, nbdevdn}; upper, middle, lower; L = p-1 */
    PMENV_IND_MACD = 2,    /* p = {fast, slow, signal} (swapped if slow < fast); macd, signal, hist; L = slow-1 + signal-1 */
    PMENV_IND_ATR = 3,     /* p = {timeperiod};                       L = p */
    PMENV_IND_RSI = 4,     /* p = {timeperiod};                       L = p */
    PMENV_IND_ADX = 5,     /* p = {timeperiod};                       L = 2p-1 */
    PMENV_IND_DX = 6,      /* p = {timeperiod};                       L = p */
    PMENV_IND_STOCH = 7,   /* p = {fastk, slowk, slowd};              slowk, slowd; L = the three periods - 3 */
    PMENV_IND_CCI = 8,     /* p = {timeperiod};                       L = p-1 */
    PMENV_IND_OBV = 9,     /* no parameter;                           L = 0 */
    PMENV_IND_ADOSC = 10   /* p = {fast, slow};                       L = max(fast, slow) - 1 */
} pmenv_ind_kind;
typedef struct pmenv_ind_op {
    int32_t kind;          /* pmenv_ind_kind */
    int32_t p[3];          /* the periods, each 2 .. 256; unused entries are ignored */
    double f[2];           /* bbands: the band multipliers */
} pmenv_ind_op;
/* *n_out = K, the output columns of the ops in order; *lookback = L, the largest lookback
 * (either may be NULL). Host only. PMENV_ERR_ARG: NULL ops, n_ops outside 1 .. 32, an unknown
 * kind, a period outside 2 .. 256, a band multiplier that is not finite. */
int pmenv_ind_layout(const pmenv_ind_op* ops, int32_t n_ops, int32_t* n_out, int32_t* lookback);
/* Device scratch of one call in bytes: the split form's segment records and stoch's fastk
 * stream. May be 0 for a valid call; 0 for a refused shape too. */
size_t pmenv_ind_workspace(int32_t T, int32_t N, const pmenv_ind_op* ops, int32_t n_ops);
/* out[(r * N + n) * ldo + col0 + k] = output k of the call at series row L + r, for r < T - L,
 * n < N, k < K: every op is aligned to the call's lookback, and nothing else of out is
 * written (ldo > K leaves the other channels of a combined [T - L, N, ldo] tensor alone).
 * chan[5] = the channels of open, high, low, close, volume in bars; -1 for one no op needs.
 * Windowed values (sums, sums of squares, max, min, mean absolute deviation over the trailing
 * p rows) are one ascending f64 chain per output and depend on no geometry; the recurrences
 * (EMA, Wilder average and sum, running sum) run one lane per column over all rows
 * (ind_scan_seq_kernel) or, for few columns, over row segments whose carries are composed in
 * order (ind_scan_split_kernel) — pmenv_ind_path names the choice. The split form's carries
 * differ from the sequential chain by ~1e-16 of a state's magnitude: outputs agree to the f32
 * bit except where an output is the difference of two states that have converged on one value
 * (adosc on a flat A/D line, macd on a constant close), which is rounding noise in either form.
 * A NaN or inf follows IEEE
 * through the definitions: it poisons the windowed outputs that read it and its column's
 * recurrences from that row on, never another column. PMENV_ERR_ARG: what pmenv_ind_layout
 * refuses, T <= L, N < 1, a needed channel that is -1 or >= C, col0 < 0 or col0 + K > ldo, out
 * overlapping bars, and, when pmenv_ind_workspace is not 0, NULL work, work not 8-B aligned
 * or work_bytes below it. PMENV_ERR_ALIGN: bars or out not 4-B aligned. The result does not depend on
 * what work held. No allocation, no synchronisation, capturable. */
int pmenv_ind_apply(const float* bars, int32_t T, int32_t N, int32_t C, const int32_t chan[5],
                    const pmenv_ind_op* ops, int32_t n_ops, float* out, int32_t ldo, int32_t col0, void* work,
                    size_t work_bytes, hipStream_t stream);
/* The kernels of that call in launch order with their geometry, " | " between them, e.g.
 *   "ind_scan_split_kernel walks=1 seg=78 segs=64 grid=8x64 block=64 | ind_fastk_kernel grid=9961 block=256 | ind_window_kernel ops=3 grid=9896 block=256"
 * walks: launches of the recurrences (one op of each kind per walk); seg / segs: rows per
 * segment and segments. "" for a refused shape. Host only; thread-local, valid until the
 * thread's next call; read from the plan pmenv_ind_apply dispatches on. */
const char* pmenv_ind_path(int32_t T, int32_t N, const pmenv_ind_op* ops, int32_t n_ops);

/* ---- the search for the orders of differencing on the device (data/ffd.py:59-78,
 * FixedFracDiff.fit: per (ticker, feature) column a bisection of d whose every probe is one
 * conv1d (:69) and one statsmodels adfuller call (:70) on the host; the reference caches the
 * result in its d_opt pickles). statsmodels is not a dependency and parity with it is not
 * pinned: the definitions below are the contract (DESIGN.md "The ADF search" restates them).
 *
 * The ADF statistic of a column x[0 .. n-1] (widened to f64) is adfuller(x) at its defaults,
 * regression "c", autolag "AIC": D[i] = x[i+1] - x[i]; the model of lag k on rows i = s .. n-2
 * is D[i] = alpha + beta x[i] + sum_{j=1..k} gamma_j D[i-j] + eps. maxlag = min(n / 2 - 2,
 * ceil(12 (n / 100)^(1/4))), the ceiling taken in integers (the smallest m with 100 m^4 >=
 * 20736 n); a caller's maxlag >= 0 replaces the rule and is clamped to n / 2 - 2. With autolag
 * the lags k = 0 .. maxlag are all fitted on the common rows s = maxlag, nobs = n - 1 - maxlag,
 * AIC_k = nobs ln(ssr_k / nobs) + 2 (k + 2), and usedlag is the smallest k of the smallest AIC;
 * without it usedlag = maxlag. The final fit has lag usedlag on rows s = usedlag, nobs = n - 1 -
 * usedlag, p = usedlag + 2 parameters, and stat = beta / sqrt(ssr / (nobs - p) [(X'X)^-1]_beta).
 * The p-value is MacKinnon's (1994) for a constant and one series: 1 above 2.74, 0 below
 * -18.83, Phi(2.1659 + 1.4412 s + 0.038269 s^2) up to -1.61 and Phi(1.7339 + 0.93202 s -
 * 0.12745 s^2 - 0.010368 s^3) above, Phi(z) = erfc(-z / sqrt 2) / 2 in f64. ---- */
typedef enum pmenv_adf_status {
    PMENV_ADF_OK = 0,
    PMENV_ADF_TOO_SHORT = 1,   /* n < 16: stat and pvalue NaN, usedlag and nobs 0 */
    PMENV_ADF_DEGENERATE = 2   /* a value that is not finite, a pivot that is not positive or an ssr <= 0 in any
                                  fit (a constant column, a pure ramp): stat and pvalue NaN, usedlag and nobs 0 */
} pmenv_adf_status;
/* ffd.py:38-47 for every column at once, on the device: d [C] f64 -> taps [cap, C] f32
 * (tap-major, rows >= width[c] zeroed) and width [C] int32, the taps and the width of
 * pmenv_ffd_weights(d[c], thres, T) bit for bit (one lane per column runs the same f32 factors
 * and f64 running product; min(width, cap) taps are written). A d[c] that is negative or not
 * finite gives width 0. PMENV_ERR_ARG: NULL d or width, T < 2, C < 1, cap < 0, NULL taps with
 * cap > 0, thres negative or not finite. d 8-B, taps and width 4-B aligned. No allocation, no
 * synchronisation, capturable. */
int pmenv_ffd_table(const double* d, double thres, int32_t T, int32_t C, int32_t cap, float* taps, int32_t* width,
                    hipStream_t stream);
/* The lag bound of a column of n rows (the integer rule above; maxlag < 0: the default) and
 * the p-value of a statistic, as the kernels compute them. Host only. */
int32_t pmenv_adf_maxlag(int64_t n, int32_t maxlag);
double pmenv_adf_pvalue(double stat);
/* Device scratch of one pmenv_adf call in bytes: 2 kcap + 7 doubles per column, kcap the lag
 * bound of a column of R rows. 0 for a refused shape. */
size_t pmenv_adf_workspace(int32_t R, int32_t C, int32_t maxlag);
/* ffd.py:70 (adfuller(...)[1]) for every column of y [R, C] f32 (row stride ld >= C floats) in
 * two launches. Column c is rows first[c] .. R-1 (first NULL: 0; clamped to [0, R]), so
 * columns of unequal length — the outputs of filters of unequal width — share one tensor.
 * maxlag < 0: the default rule per column; autolag 0: usedlag = maxlag. stat, pvalue f64 [C],
 * usedlag, nobs, status (pmenv_adf_status) int32 [C].
 * The fits are solved through the normal equations in f64: level and differences are shifted
 * by constants near their means (the mean of 64 evenly spread rows; (x[n-1] - x[0]) / (n - 1)), the Gram matrix of [level, D_-1 .. D_-maxlag | D] is
 * centred by the column sums over the fit's rows (the constant absorbs the means) and factored
 * once (Cholesky); the models are nested in that order, so every ssr_k comes from that one
 * factor. The final fit adds the maxlag - usedlag earlier rows and factors once more. Every sum
 * is one chain in a fixed order: a column's outputs depend on no other column, not on C, ld or
 * first[c], and not on what work held. A NaN or inf touches its own column only (DEGENERATE).
 * PMENV_ERR_ARG: a NULL pointer other than first, R < 1, C < 1, ld < C, maxlag > 64 or a
 * default lag bound above 64 (R > 80,908), work NULL, not 8-B aligned or below
 * pmenv_adf_workspace. PMENV_ERR_ALIGN: y, first or an int32 output not 4-B, stat or pvalue
 * not 8-B aligned. No allocation, no synchronisation, capturable. */
int pmenv_adf(const float* y, int32_t R, int32_t C, int32_t ld, const int32_t* first, int32_t maxlag,
              int32_t autolag, double* stat, double* pvalue, int32_t* usedlag, int32_t* nobs, int32_t* status,
              void* work, size_t work_bytes, hipStream_t stream);
/* The kernels of that call in launch order with their geometry, e.g.
 *   "adf_sums_kernel tile=8 chunk=256 kcap=17 grid=17 block=512 | adf_solve_kernel kcap=17 lds=3952 grid=130 block=64"
 * tile: columns per workgroup of the sums (one wave each), chunk: rows per staging step, kcap:
 * the largest lag bound of the call, lds: dynamic LDS bytes. "" for a refused shape. Host
 * only; thread-local, valid until the thread's next call. */
const char* pmenv_adf_path(int32_t R, int32_t C, int32_t maxlag);
/* One round of ffd.py:59-78 for every column, one thread each, on the state low, high, d_opt
 * (f64 [C]; 0, 1, 0 at the start) and active, evals, status (int32 [C]). pvalue NULL: the
 * first round, nothing probed yet. Otherwise an active column's probe at d_opt gave pvalue[c],
 * stat[c], adf_status[c]: status[c] takes the probe's status and last [2, C] (may be NULL) its
 * pvalue and stat; TOO_SHORT counts as p = 1 (the reference would raise: the one deliberate
 * deviation); p > 0.05 sets low = d_opt, p < 0.049 sets high = d_opt, anything else (the band,
 * a NaN) ends the column at d_opt (:73-78). A column still active takes d_mid = (low + high) /
 * 2: d_mid < thres ends it at d_opt = 0 (:62-64), |d_opt - d_mid| < thres ends it where it is
 * (:65-66), otherwise d_opt = d_mid is its next probe and evals[c] grows by one. d[c] = d_opt
 * for every column, active or not. Every d is a dyadic rational: the trajectory is exact.
 * PMENV_ERR_ARG: a NULL state pointer or d, C < 1, thres not positive, pvalue without stat and
 * adf_status. No allocation, no synchronisation, capturable. */
int pmenv_adf_search_update(const double* pvalue, const double* stat, const int32_t* adf_status, double thres,
                            int32_t C, double* low, double* high, double* d_opt, int32_t* active, int32_t* evals,
                            int32_t* status, double* last, double* d, hipStream_t stream);

/* ---- trainer-side twin: the differentiable batched portfolio reward of the
 * PG / A2C agents (agent/pg/pg.py:40-82 `_reward`, agent/a2c.py/a2c.py:40-82 `_loss`
 * = -_reward), forward and backward in f64 over a [B, N] batch. ---- */
typedef enum pmenv_batch_norm {
    PMENV_BNORM_GLOBAL_OR = 0, /* reference: softmax over assets iff !isclose(sum over the WHOLE batch, 1)
                                  OR min < 0 (pg.py:52) */
    PMENV_BNORM_ROW_OR = 1,    /* the same decision per row */
    PMENV_BNORM_NONE = 2
} pmenv_batch_norm;

/* f64 scratch the forward fills and the backward reads: (6*B + 8 + 16*ceil(B/16)) * 8 bytes. */
size_t pmenv_batch_reward_workspace(int32_t B);
/* a, p [B, N]; v_prev [B] (the _v of pg.py); reward_kind LOG_RETURN / RETURN / SHARPE
 * (batch mean / std, pg.py:80); writes reward_out[0] (device) and optionally the
 * per-row gross returns ret_out [B]. a, p and grad_a need 4-B alignment only, work 8-B.
 * Limit: B * N * 4 < 2^32 (the kernels address a, p and grad_a through 32-bit byte
 * offsets; a larger batch is the caller's to split). */
int pmenv_batch_reward_forward(const float* a, const float* v_prev, const float* p, int32_t B, int32_t N,
                               int32_t reward_kind, int32_t norm, double scale, double* work,
                               float* reward_out, float* ret_out, hipStream_t stream);
/* grad_a [B, N] = grad_out[0] * dR/da (grad_out is a device scalar). */
int pmenv_batch_reward_backward(const float* a, const float* v_prev, const float* p, int32_t B, int32_t N,
                                int32_t reward_kind, double scale, const double* work,
                                const float* grad_out, float* grad_a, hipStream_t stream);
/* The kernels a [B, N] batch takes, as a string of three fields joined by " | ": the
 * forward's row kernel with its template argument (elements per lane; 0: the looping form),
 * the backward kernel, and "parts=K", the number of partial records the forward's fold reads:
 *   "batch_reward_small_kernel<8> | batch_reward_grad_quad_kernel<8> | parts=1"       (64 x 30)
 *   "batch_reward_rows_quad_kernel<16> | batch_reward_grad_quad_kernel<16> | parts=2" (65 x 33)
 *   "batch_reward_rows_kernel<0> | batch_reward_grad_kernel<0> | parts=1"             (3 x 700)
 * (the small kernel folds its one record in the same launch; the others are followed by
 * batch_reward_final_kernel and, with ret_out, batch_reward_select_kernel). "" for B < 1 or
 * N < 1. The entry points above dispatch on the same decision. Host only: launches nothing,
 * touches no device; the string is thread-local and valid until the thread's next call. */
const char* pmenv_batch_reward_path(int32_t B, int32_t N);

/* ---- device replay and trajectory metrics ---- */

/* replay/buffer.py:39-79 ReplayBuffer.sample for vectorised envs over a ring of H
 * recorded steps (days [H, B] int32 = last day of the window acted on, actions
 * [H, B, N], rewards [H, B]): for each of the S samples (h0[j], env[j]) writes
 * s, s_next [S, N, W, F] (market channels from series [T, N, F-1], channel F-1 = the
 * W actions h0..h0+W-1, resp. h0+1..h0+W), a_out [S, N] = actions[h0+W],
 * r_out [S] = rewards[h0+W-1]. Days outside the series read NaN. */
int pmenv_replay_gather(const float* series, int32_t T, int32_t N, int32_t F, int32_t W,
                        const int32_t* days, const float* actions, const float* rewards,
                        int32_t H, int32_t B, const int32_t* h0, const int32_t* env, int32_t S,
                        float* s, float* s_next, float* a_out, float* r_out, hipStream_t stream);

/* The n-step sample of the same ring: agent/td3/td3.py:85-106 (add_experience) folds the
 * last n_step transitions into one before it stores them — reward = r + gamma * reward *
 * (1 - d) from the back (:94-96), the first state and action, the next state of the step
 * where the fold stopped; here every step is already recorded (replay/buffer.py:39-79),
 * so the fold happens at sample time. The ring holds `count` <= H recorded rows, the
 * oldest at row `oldest`; row h has position (h - oldest) mod H. row_episode [H] int32
 * is each row's episode id, not decreasing from the oldest row to the newest (NULL = one
 * episode). For a valid one-step sample (h0[j], env[j]) at position st, m is the largest
 * count in [1, n] such that st + m - 1 < count - W - 1 and rows st .. st + m - 1 + W share
 * one episode (td3's `done`: an episode boundary or the newest rows end the fold early).
 * Writes s, a_out as pmenv_replay_gather does; s_next = that call's s_next for the start
 * h0 + m - 1 (the window ending at days[h0+m+W-2] + 1, channel F-1 = actions h0+m ..
 * h0+m+W-1); r_out [S] = sum_{k<m} gamma^k rewards[h0+W-1+k], Horner from the last term
 * in f64, rounded once; steps [S] = m; discount [S] = gamma^m (f64 product). n = 1 is
 * pmenv_replay_gather bit for bit. PMENV_ERR_ARG: n < 1, count > H, oldest outside
 * [0, H), gamma outside (0, 1], a NULL pointer other than row_episode. */
int pmenv_replay_gather_nstep(const float* series, int32_t T, int32_t N, int32_t F, int32_t W,
                              const int32_t* days, const float* actions, const float* rewards,
                              int32_t H, int32_t B, const int32_t* h0, const int32_t* env, int32_t S,
                              const int32_t* row_episode /* [H], NULL = one episode */,
                              int32_t oldest, int32_t count, int32_t n, float gamma,
                              float* s, float* s_next, float* a_out, float* r_out,
                              int32_t* steps, float* discount, hipStream_t stream);

/* Sequence samples of the same ring (agent/dreamer/dreamer.py:77-80 trains on sequences of
 * consecutive steps; world_model.py:41-64 walks them time-major). Element t of sequence j
 * is the one-step sample at start (h0[j] + t) mod H of env[j] as pmenv_replay_gather
 * defines it: x = its s, a_out = its a_out (actions[h0+t+W]), r_out = its r_out
 * (rewards[h0+t+W-1]). length [S] = m, the n-step count of pmenv_replay_gather_nstep with
 * n = L: an episode boundary or the newest rows cut a sequence short. Elements t >= m are
 * written as +0.0 in x, a_out and r_out. Each element takes the window ending at its own
 * days[h0+t+W-1], so a ring whose day indices skip is served too; days outside the series
 * read NaN. time_major != 0: x [L, S, N, W, F], a_out [L, S, N], r_out [L, S] (Dreamer's
 * order); time_major == 0: x [S, L, N, W, F], a_out [S, L, N], r_out [S, L]. Enqueues on
 * `stream`; never synchronises, allocates or frees. PMENV_ERR_ARG: L < 1, count > H,
 * oldest outside [0, H), a NULL pointer other than row_episode, the shape errors of
 * pmenv_replay_gather_nstep. */
int pmenv_replay_gather_seq(const float* series, int32_t T, int32_t N, int32_t F, int32_t W,
                            const int32_t* days, const float* actions, const float* rewards,
                            int32_t H, int32_t B, const int32_t* h0, const int32_t* env, int32_t S,
                            const int32_t* row_episode /* [H], NULL = one episode */,
                            int32_t oldest, int32_t count, int32_t L, int32_t time_major,
                            float* x, float* a_out, float* r_out, int32_t* length, hipStream_t stream);

/* ---- per-env episodes: a replay fed by envs that restart on their own (pmenv_restart_days)
 * keeps env_episode [H, B] int32, the episode id of ring row h for env b, not decreasing
 * from the oldest row to the newest in every column b. replay/buffer.py:47-59 draws a start
 * inside one epoch of its [epoch, step] layout and reads the window's rows from that epoch
 * alone; here "rows st .. st + need - 1 of env b share one episode" is decided per column,
 * by the first and the last of those rows. need = W + 1 for a one-step or n-step start
 * (agent/td3/td3.py:94-97 stops its fold at `done`), W + L for a full-length sequence
 * (agent/dreamer/dreamer.py:77-80); span = max(count - need, 0) start offsets exist. ---- */

/* The map of valid (start, env) pairs (replay/buffer.py:47-59: the starts a draw may
 * take). bits [span][ceil(B / 64)] u64: bit b & 63 of word (st, b >> 6) is set iff
 * env_episode[(oldest + st) % H, b] == env_episode[(oldest + st + need - 1) % H, b]; the bits at and beyond B of a row's last word are 0. rowsum [span + 1]
 * int64: rowsum[0] = 0, rowsum[st + 1] - rowsum[st] = the set bits of row st, rowsum[span] =
 * the total. Integer arithmetic only: the same bits whatever the dispatch order. span == 0
 * writes rowsum[0] alone (bits may then be NULL). Both buffers 8-byte aligned
 * (PMENV_ERR_ALIGN). Enqueues two launches on `stream`; never synchronises or allocates.
 * PMENV_ERR_ARG: need < 1, count outside [0, H], oldest outside [0, H), a NULL pointer. */
int pmenv_replay_valid_build(const int32_t* env_episode, int32_t H, int32_t B, int32_t oldest, int32_t count,
                             int32_t need, uint64_t* bits, int64_t* rowsum, hipStream_t stream);
/* S exact draws from that map (replay/buffer.py:47-59 draws the epoch, the start and the
 * env uniformly; here the pair is uniform over the valid set): with total = rowsum[span],
 * sample j takes k = clamp(floor(u[j] * total), 0, total - 1), u [S] f64, a NaN u counting
 * as 0, and writes the k-th valid pair in (st ascending, env ascending) order as h0[j] =
 * (oldest + st) % H and env[j]. total == 0 writes -1 to both for every sample and reads no
 * bits. One launch, one wave per sample. */
int pmenv_replay_valid_select(const uint64_t* bits, const int64_t* rowsum, int32_t H, int32_t B, int32_t oldest,
                              int32_t span, const double* u, int32_t S, int32_t* h0, int32_t* env,
                              hipStream_t stream);
/* pmenv_replay_gather_nstep with env_episode [H, B] in place of row_episode [H]
 * (agent/td3/td3.py:94-97: the fold of sample (h0[j], env[j]) stops where env[j]'s episode
 * ends): m is decided by column env[j]. The same argument errors and the same plan
 * (pmenv_replay_path); the plan's F = 5 persistent kernel runs in its build for the [H, B]
 * id layout (replay_nstep_f5p_env_kernel, replay_seq_f5p_env_kernel: the same template
 * arguments and geometry), the other forms take the layout as strides. NULL = one episode. */
int pmenv_replay_gather_nstep_env(const float* series, int32_t T, int32_t N, int32_t F, int32_t W,
                                  const int32_t* days, const float* actions, const float* rewards,
                                  int32_t H, int32_t B, const int32_t* h0, const int32_t* env, int32_t S,
                                  const int32_t* env_episode /* [H, B], NULL = one episode */,
                                  int32_t oldest, int32_t count, int32_t n, float gamma,
                                  float* s, float* s_next, float* a_out, float* r_out,
                                  int32_t* steps, float* discount, hipStream_t stream);
/* pmenv_replay_gather_seq likewise (agent/dreamer/dreamer.py:77-80: a sequence lies in one
 * episode of its env): length[j] is decided by column env[j]. */
int pmenv_replay_gather_seq_env(const float* series, int32_t T, int32_t N, int32_t F, int32_t W,
                                const int32_t* days, const float* actions, const float* rewards,
                                int32_t H, int32_t B, const int32_t* h0, const int32_t* env, int32_t S,
                                const int32_t* env_episode /* [H, B], NULL = one episode */,
                                int32_t oldest, int32_t count, int32_t L, int32_t time_major,
                                float* x, float* a_out, float* r_out, int32_t* length, hipStream_t stream);

/* The kernel and the launch geometry a sample gather takes for a shape, from the plan the
 * gathers themselves switch on. kind: which gather (PMENV_REPLAY_ROLLOUT: pmenv_rollout_gather,
 * declared below); n: pmenv_replay_gather_nstep's n or pmenv_replay_gather_seq's L (ignored by
 * the other two); aligned: bit 0 = the window outputs (s, s_next / x) are 16-B aligned, bit 1
 * = series is; cus: the device's compute units, <= 0 for the calling process's current device
 * (with a count given the call touches no device). Returns a thread-local string, valid
 * until the thread's next call: the kernel's name as the library instantiates it, then
 * space-separated R= (asset rows per group, 0 for a form without groups), D= (staged days)
 * and Lc= nc= (elements per chunk, chunks per sequence) where the form has them, grid=XxY
 * and lds= (dynamic LDS bytes), e.g. "replay_seq_f5p_kernel<8,16> R=30 D=54 Lc=4 nc=16
 * grid=256x1 lds=32416"; "" for a shape the gather rejects or an unknown kind. Host only:
 * launches nothing. */
typedef enum pmenv_replay_kind {
    PMENV_REPLAY_ONE_STEP = 0,
    PMENV_REPLAY_NSTEP = 1,
    PMENV_REPLAY_SEQ = 2,
    PMENV_REPLAY_ROLLOUT = 3
} pmenv_replay_kind;
const char* pmenv_replay_path(int32_t kind, int32_t N, int32_t F, int32_t W, int32_t n, int32_t S,
                              int32_t aligned, int32_t cus);

/* ---- prioritized sampling over the same ring. agent/td3/td3.py:39 builds
 * PrioritizedReplayBuffer(buffer_size, alpha, beta, beta_incr), :118 reads `samples, idxs,
 * weights = replay_buffer.sample(batch_size)`, :126,143 weight the critic loss and :144
 * calls update_priorities(idxs, td_error). The module td3.py:12 imports is not in the
 * reference tree, so parity is unpinned; the definitions are those of Schaul et al. 2016,
 * "Prioritized Experience Replay", proportional variant: P(j) = p_j^alpha / sum_k p_k^alpha,
 * w_j = (N P(j))^-beta / max_k w_k, p_j = |td_j| + eps, new transitions enter at the largest
 * priority seen.
 *
 * The tree is a radix-64 sum tree over `leaves` = H * B leaves, 1 <= leaves < 2^31. Leaf
 * l = h * B + b is the one-step sample that starts at ring row h of env b; it is an f32 and
 * holds p^alpha, and it is 0 exactly when (h, b) is not a valid one-step start. Level 0 is
 * the leaves, n_0 = leaves; level k >= 1 has n_k = ceil(n_{k-1} / 64) f64 nodes, node i the
 * sum of entries [64 i, 64 i + 64) of level k - 1 that exist; the levels end with the first
 * k >= 1 that has n_k <= 64 (so there is always a level 1). One caller-owned device buffer
 * of pmenv_prio_tree_bytes(leaves) bytes, 8-byte aligned (PMENV_ERR_ALIGN), holds
 *
 *     [0, 64)                        header: f32 at byte 0 = the running maximum leaf value
 *     [64, 64 + 4 * pad(n_0))        the leaves (f32)
 *     then for k = 1, 2, ..          level k: 8 * pad(n_k) bytes (f64)
 *
 * with pad(n) = 64 * ceil(n / 64): every level is padded with zeros, which the calls never
 * change. Every call validates its arguments (PMENV_ERR_ARG), enqueues a linear chain of
 * launches on `stream`, never allocates, frees or synchronises, may be captured in a
 * hipGraph, and is deterministic: a touched node is recomputed from its 64 children in a
 * fixed order, there are no floating-point atomics, and the same inputs give the same bits
 * whatever the dispatch order. ---- */
size_t pmenv_prio_tree_bytes(int64_t leaves); /* 0 when leaves is outside [1, 2^31) */
/* Every leaf and node 0, the maximum 1. */
int pmenv_prio_init(void* tree, int64_t leaves, hipStream_t stream);
/* Leaves [close_first, close_first + n) become 0 and leaves [open_first, open_first + n)
 * the current maximum; every ancestor is refreshed. A negative first = that range is
 * absent. The ranges must lie inside the leaves and must not overlap. The replay calls it
 * once per recorded step with n = B: the ring row just overwritten closes and the row whose
 * window became complete opens. */
int pmenv_prio_fill(void* tree, int64_t leaves, int64_t close_first, int64_t open_first, int64_t n,
                    hipStream_t stream);
/* pmenv_prio_fill for per-env episodes (replay/buffer.py:47-59: a start is valid inside one
 * episode of its env): leaf open_first + i opens only where ep_first[i] == ep_last[i], i in
 * [0, n) — the two rows of env_episode at the start's first and last ring row; the other
 * leaves of the open range keep their value (0: their row's close). The close range is
 * pmenv_prio_fill's. PMENV_ERR_ARG also for a NULL ep_first / ep_last with an open range. */
int pmenv_prio_fill_env(void* tree, int64_t leaves, int64_t close_first, int64_t open_first, int64_t n,
                        const int32_t* ep_first, const int32_t* ep_last, hipStream_t stream);
/* S samples (td3.py:118). Sample j takes the target u[j] * total, u[j] in [0, 1) (f64),
 * total = the sum of the top level in the order the descent scans it (a 64-lane prefix
 * scan). At each node the first child with a positive value whose inclusive prefix exceeds
 * the residual is chosen and its exclusive prefix subtracted; a child of value 0 is never
 * chosen; if rounding leaves the residual at or above the node's sum, the last child with a
 * positive value is taken. leaf_out [S] = the leaf, h0_out = leaf / B, env_out = leaf % B
 * (ready for the gathers above), weight_out [S] = (leaf_j / min_k leaf_k)^-beta over the
 * batch's leaf values, in f64, rounded once. That is the paper's (N P(j))^-beta / max_k w_k:
 * N and total cancel under the batch-max normalisation, and the largest weight is exactly
 * 1. An empty tree gives leaf 0 and weight 0. beta >= 0. */
int pmenv_prio_sample(const void* tree, int64_t leaves, int32_t B, const double* u, int32_t S, float beta,
                      int32_t* leaf_out, int32_t* h0_out, int32_t* env_out, float* weight_out,
                      hipStream_t stream);
/* update_priorities (td3.py:144): leaf[j] takes max((|td[j]| + eps)^alpha, FLT_MIN),
 * computed in f64, rounded once to f32 and capped at FLT_MAX; a non-finite td gives the
 * maximum the header held when the call began. A leaf that is 0 stays 0 (its row was
 * overwritten or closed since it was sampled) and its ancestors keep their bits. Where
 * leaf[] repeats an index the largest new value wins, whatever the order; the old value is
 * no candidate. The header's maximum becomes max(old, every finite new value). Every
 * ancestor of a touched leaf is refreshed, level by level. Indices outside [0, leaves) are
 * skipped. alpha >= 0, eps >= 0. */
int pmenv_prio_update(void* tree, int64_t leaves, const int32_t* leaf, const float* td, int32_t S,
                      float alpha, float eps, hipStream_t stream);

/* The compact on-policy rollout (replay/rollout_buffer.py:43-57 stores s per step;
 * here the windows are re-materialised instead): for each of the S
 * samples (t_idx[j], env[j]) writes s[j] = env b's window after t updates, [N, W, F]:
 * market channels from series [T, N, F-1] at days start[b] + t .. start[b] + t + W - 1
 * (start [B] = first day of the reset window; days outside read NaN), channel F-1 =
 * ActionBuffer.get_all() rebuilt from the post-drift weights [T_rec, B, N] of updates
 * 1 .. T_rec (weight_buffer.py:32-44; ring_mode = pmenv_ring_mode). t_idx <= T_rec. */
int pmenv_rollout_gather(const float* series, int32_t T, int32_t N, int32_t F, int32_t W, const int32_t* start,
                         const float* weights, int32_t T_rec, int32_t B, int32_t ring_mode,
                         const int32_t* t_idx, const int32_t* env, int32_t S, float* s, hipStream_t stream);

/* The per-env form of the compact rollout: envs that restart on their own
 * (pmenv_restart_days) and rollouts that continue from where the last one stopped. For every
 * buffer row t = 0 .. T_rec and env b two int32 arrays [T_rec + 1, B] describe the window env
 * b holds after step t:
 *   first[t, b]    the series day of the window's first day (restart[b] after a restart);
 *   updates[t, b]  the ring updates since the env's last reset at that moment, 0 for a window
 *                  a reset or a restart just wrote.
 * weights is [carry + T_rec, B, N]: the post-drift weights w' of step g (1 <= g <= T_rec) sit
 * in row carry + g - 1, rows 0 .. carry - 1 hold the w' of the `carry` steps before this
 * rollout began (carry = 0, or W when a rollout resumes). The lockstep case is
 * first = start[b] + t, updates = t, carry = 0, and gives pmenv_rollout_gather's bits.
 * The window (t, b), with u = updates[t, b]:
 *   market channels f < F-1 read series[first[t, b] + p, n, f], NaN outside the series;
 *   the weight channel at window position p has chronological position c = p, or, in
 *   PMENV_RING_STORAGE mode with u >= W-1, c = (p - u - 1) mod W; its episode-local history
 *   row is r = u + c: r < W-1 reads 0, r == W-1 reads e0 (1 for asset 0, else 0), r > W-1
 *   reads the w' of step g = t + c - W + 1, weights row carry + t + c - W.
 * The caller keeps t_idx <= T_rec and updates[t, b] <= t + carry, so that a row r > W-1 lies
 * in weights (with carry >= W every position has its row, whatever u is: an env that never
 * restarts may run on across resumed rollouts); a weights row outside [0, carry + T_rec)
 * reads 0.0f, never memory. The same plan as pmenv_rollout_gather (form,
 * grid, LDS bytes, store policy) with the kernels rollout_gather_env_tile_kernel /
 * rollout_gather_env_rows_kernel; enqueues on `stream`, never allocates, frees or
 * synchronises (capturable). PMENV_ERR_ARG: a NULL pointer, carry < 0, or
 * pmenv_rollout_gather's shape errors. */
int pmenv_rollout_gather_env(const float* series, int32_t T, int32_t N, int32_t F, int32_t W,
                             const int32_t* first, const int32_t* updates, const float* weights, int32_t carry,
                             int32_t T_rec, int32_t B, int32_t ring_mode, const int32_t* t_idx,
                             const int32_t* env, int32_t S, float* s, hipStream_t stream);
/* pmenv_replay_path(PMENV_REPLAY_ROLLOUT, ...)'s string with the per-env kernels' names; "" for
 * a shape the gather rejects. Host only: launches nothing, touches no device. */
const char* pmenv_rollout_gather_env_path(int32_t N, int32_t F, int32_t W, int32_t S, int32_t aligned);

/* util/eval.py:14-37 per env over a trajectory: returns [T, B] (simple returns),
 * values [T+1, B] f64, weights [T+1, B, N]; out [B, 5] f64 =
 * {sharpe, sortino, max drawdown, average turnover, final value} from f64 simple
 * returns [T, B], values [T+1, B] f64 and weights [T+1, B, N] f32, quantstats
 * definitions with per-period risk-free (1+rf)^(1/periods)-1 (parity unpinned:
 * quantstats is absent). */
int pmenv_metrics(const double* returns, const double* values, const float* weights, int32_t T, int32_t B,
                  int32_t N, double risk_free_rate, double periods, double* out, hipStream_t stream);

/* The same five metrics per episode, for envs that end their episodes on their own
 * (pmenv_restart_days): the reference's Metrics are per episode ("walk the series to its end",
 * then metrics.write(), train/off_policy.py:96-110).
 *
 * A record of T consecutive steps of B envs; steps are t = 1 .. T:
 *   returns    [T, B] f64      row t-1 is step t's simple return;
 *   values     [T+1, B] f64    row 0 is the value before step 1, row t the value after step t;
 *                              where step t ended an episode this is the terminal value, copied
 *                              before the restart overwrote it (as DeviceRolloutBuffer.add does);
 *   weights    [T+1, B, N] f32 post-drift weights, same rows as values;
 *   dones      [T, B] uint8    row t-1 nonzero (any nonzero byte) means step t ended env b's
 *                              episode: the layout pmenv_gae and episodes.collect use;
 *   init_value f64             the value every restarted env begins from.
 * The weights a restarted env begins from are e0 (1 for asset 0, else 0).
 *
 * Segments of env b. Let d_1 < .. < d_m be the steps with a nonzero done and e_0 = 0. Segment
 * k (0-based) covers steps first = e_k + 1 .. last = e_{k+1}, with e_{k+1} = d_{k+1}; if
 * d_m < T, or m = 0, one last open segment ends at T. count[b] is the number of segments,
 * always >= 1; n = last - first + 1.
 *
 * Per segment, pmenv_metrics' definitions applied to the segment:
 *   x_t = returns[t-1, b] - rfp for t in the segment, rfp = (1 + rf)^(1/periods) - 1, or 0
 *   when rf = 0;
 *   sharpe  = mean(x) / std(x, ddof = 1) * sqrt(periods);
 *   sortino = mean(x) / sqrt(sum min(x, 0)^2 / n) * sqrt(periods);
 *   value path P = [V0, values[first .. last, b]], V0 = values[0, b] for k = 0, else init_value;
 *   max drawdown = min(0, min_i (P_i / max_{j <= i} P_j - 1));
 *   average turnover = sum_{t = first .. last} sum_n |weights[t, b, n] - prev| / n, prev =
 *   weights[t-1, b, n], except at t = first of a segment with k > 0, where prev is e0;
 *   final value = values[last, b]: a copy, bit-equal.
 *
 * Outputs, padded to the caller's cap K = max_episodes (no allocation, no prefix sum over
 * envs, no host read): out [B, K, 5] f64 in pmenv_metrics' field order, span [B, K, 2] int32 =
 * {first, last}, count [B] int32. Segments k < min(count[b], K) are stored in chronological
 * order; slots count[b] <= k < K get NaN in out and {0, 0} in span; count[b] is exact even when
 * it exceeds K (the first K segments are kept). A stored segment is closed iff
 * dones[last - 1, b] != 0. No atomics: the same bits on every call and for every K.
 *
 * Enqueues one launch on `stream`; never allocates, frees or synchronises (capturable).
 * PMENV_ERR_ARG: a NULL pointer, max_episodes < 1, or pmenv_metrics' shape errors. */
int pmenv_metrics_episodes(const double* returns, const double* values, const float* weights,
                           const uint8_t* dones, int32_t T, int32_t B, int32_t N, double init_value,
                           double risk_free_rate, double periods, int32_t max_episodes, double* out,
                           int32_t* span, int32_t* count, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PMENV_H */
