// handle.h — the env handle (struct pmenv) and the helpers of the host side that need HIP,
// shared by the product library (pmenv.hip, launch.h) and the tools build
// (tools/ab/pmenv_ab.hip). The handle is its shape plan (pmenv_host::StepPlan, step_plan.h:
// every field that is a function of the cfg, host only) plus what the struct below declares:
// the device memory, its streams and events, and the state that changes from step to step.
//
// The tools build — tools/libpmenv_ab.so, the A/B harnesses' library — is the product's
// translation unit linked with tools/ab/pmenv_ab.hip, which defines the pmenv_tools hooks
// below: it reads the PMENV_* knobs and launches the alternatives the product was measured
// against. The product library's definitions of the hooks (weak, at the end of pmenv.hip)
// do nothing, and it reads no environment variable.
#pragma once
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/pmenv.h"
#include "common.h"
#include "step_plan.h"

struct pmenv : pmenv_host::StepPlan {
    pmenv_cfg cfg;
    int device;
    void* state;          // value | stat_a | stat_b | counter | ring | nonfinite | last_close | w_new
    size_t state_bytes;
    bool owns_state;
    double* value;
    double* sa;
    double* sb;
    int32_t* k;
    float* ring;
    float* last_close;
    float* w_new;
    unsigned long long* nonfinite;
    float* halo;          // [halo_wgs][2] float4: first two chunks of every in-place flat workgroup
    // the flat one-launch step's copies (step_flat_kernel / step_flat_vec_kernel)
    void* snap;           // the state snapshot, two parities: value f64 | counter i32 | get_last() | last close
    double* sv[2];
    int32_t* sk[2];
    float* sw[2];
    float* slc[2];
    float* halo1[2];      // [halo1_wgs][2] float4 per parity: the next tile's first two chunks
    int par;              // parity of the snapshot / halo the next step reads
    bool snap_ok;         // sv[par] .. slc[par] equal the canonical state
    const float* halo1_obs;   // the window whose halo halo1[par] holds (null: none)
    // device-sequenced form (hipGraph-safe): from the first flat step enqueued under
    // stream capture on, every flat step is flat_seq_kernel + the kernel reading the
    // parity and the validity from seq (device words) instead of the host fields above
    bool device_seq;
    int32_t* seq;         // {D, C, V, pad, HOBS lo, HOBS hi} (step_flat.h)
    uint64_t snap_stride; // bytes between the two parities of the snapshot / halo
    // the relay step's memory and sequencing (step_relay.h)
    void* relay_mem;      // control words | relay words, deferral list, tile claims | counter copy x 2 | halo x 2 (allocated when
                          // AUTO gives the shape the relay step or pmenv_set_step_path asks for it)
    uint32_t* relay_seq;  // device-sequenced words {D, E, V, C, EC, pad, HOBS lo, HOBS hi} (step_relay.h)
    uint64_t* relay_w;    // [B * N] {epoch, w'}
    uint64_t* relay_list; // the deferral list: [0] {epoch, count}, [1 .. relay_tiles] {epoch, tile}
    uint32_t* relay_done; // [relay_tiles] the epoch in which each deferred tile last ran
    int32_t* relay_kp;    // [2][B] the counter copies, per parity
    float* relay_halo;    // in place: [2][relay_halo_stride] floats
    uint32_t relay_halo_stride;
    bool relay_kp_ok;     // eager: relay_kp[relay_par] equals the state's counter
    const float* relay_obs;   // eager: the window whose halo relay_halo[relay_par] holds (null: none)
    int relay_par;        // eager: parity of the counter copy / halo the next relay step reads
    uint32_t relay_epoch; // eager: the last step's tag
    bool relay_dseq;      // device-sequenced: from the first call of this handle enqueued under stream
                          // capture on, epoch, parity and the copies' validity live in relay_seq
    // host-I/O staging (pmenv_step_host / pmenv_reset_host): one pinned, device-mapped block,
    // allocated on the first host-I/O call — action | prices | last closes | channel [B,N,W] |
    // weights | reward (f32), then return | value (f64), then the completion words (u32);
    // `hio_dev` is its device address
    char* hio;
    char* hio_dev;
    size_t hio_off[10];
    uint32_t hio_seq;     // the last host-I/O call's completion tag
    // the resident host-I/O step (step_host_resident_kernel): its own stream, an event recorded
    // after its launch (complete = the workgroup has exited), the last tag it ran (device u32)
    hipStream_t res_stream;
    hipEvent_t res_ev;
    uint32_t* res_last;
    bool res_live;        // launched and not yet seen exited
    bool dev_pending;     // an asynchronous call of this handle since its last synchronous host call
    pmenv_dev::StepParams res_p;   // its launch arguments
    pmenv_dev::HostIO res_io;
    void* tools;        // tools build: its knob state (null in the product library)
    char err[512];
};

namespace pmenv_host {

inline void set_err(pmenv* h, const char* fmt, ...) {
    if (!h) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(h->err, sizeof(h->err), fmt, ap);
    va_end(ap);
}

struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
};

inline pmenv_dev::StepParams base_params(const pmenv* h) {
    using pmenv_dev::make_fastdiv;
    pmenv_dev::StepParams p;
    memset(&p, 0, sizeof(p));
    const pmenv_cfg& c = h->cfg;
    p.B = c.num_envs; p.N = c.num_assets; p.W = c.window; p.F = c.features;
    p.close_ch = c.close_channel;
    p.reward_kind = c.reward_kind; p.norm_mode = c.norm_mode; p.ring_mode = c.ring_mode;
    p.ret_mode = c.ret_mode; p.mu_max_iter = c.mu_max_iter;
    p.rows_per_tile = h->rows_per_tile;
    p.tile_floats = h->tile_floats;
    p.unit_rows = h->unit_rows;
    p.units_per_env = h->units_per_env;
    p.init_cash = c.init_cash; p.commission = c.commission; p.scale = c.reward_scale;
    p.rf = c.risk_free_rate; p.eta = c.sharpe_eta; p.mu_tol = c.mu_tol;
    p.value = h->value; p.k = h->k; p.ring = h->ring; p.last_close = h->last_close;
    p.w_new = h->w_new;
    p.sa = h->sa; p.sb = h->sb;
    p.nonfinite = h->nonfinite;
    p.div_wf = make_fastdiv((uint32_t)(c.window * c.features));
    p.div_f = make_fastdiv((uint32_t)c.features);
    p.div_w = make_fastdiv((uint32_t)c.window);
    p.div_units = make_fastdiv((uint32_t)(h->units_per_env > 0 ? h->units_per_env : 1));
    return p;
}

inline bool aligned4(const void* ptr) { return ((uintptr_t)ptr & 3u) == 0; }

// the current device's compute units, for the handle-less entry points that launch one
// workgroup per CU: queried once per process, 256 where the query fails
inline int device_cus() {
    static const int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        return n;
    }();
    return cus;
}

inline int check_launch(pmenv* h, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_err(h, "%s launch failed: %s", what, hipGetErrorString(e));
        return PMENV_ERR_HIP;
    }
    return PMENV_OK;
}

}  // namespace pmenv_host

// ---------------------------------------------------------------- tools-build hooks
// Defined weak (doing nothing) in pmenv.hip; tools/ab/pmenv_ab.hip defines them for
// tools/libpmenv_ab.so. A launch hook returns true when it enqueued the launch itself.
namespace pmenv_dev {
struct RelayParams;
}

namespace pmenv_tools {
void plan(pmenv* h);        // after the product's shape plan, before any allocation
void release(pmenv* h);
bool launch_scalar(const pmenv* h, const pmenv_dev::StepParams& p, hipStream_t stream);
bool launch_advance(const pmenv* h, const pmenv_dev::StepParams& p, hipStream_t stream);
bool launch_one(const pmenv* h, const pmenv_dev::StepParams& p, hipStream_t stream);
bool launch_small(const pmenv* h, const pmenv_dev::StepParams& p, hipStream_t stream);
bool launch_gen(const pmenv* h, const pmenv_dev::StepParams& p, hipStream_t stream);
bool launch_fused(const pmenv* h, const pmenv_dev::StepParams& p, int fuse_bit, uint32_t phases, hipStream_t stream);
bool launch_relay(const pmenv* h, const pmenv_dev::StepParams& p, const pmenv_dev::RelayParams& r, unsigned grid,
                  hipStream_t stream);
bool launch_flat1(const pmenv* h, const pmenv_dev::StepParams& p, unsigned grid, bool out, int pol,
                  hipStream_t stream);
bool gae(const float* rewards, const float* values, const uint8_t* dones, float* adv, float* ret, int32_t T,
         int32_t B, float gamma, float lam, hipStream_t stream, int* rc);
bool replay_gather(const float* series, int32_t T, int32_t N, int32_t F, int32_t W, const int32_t* days,
                   const float* actions, const float* rewards, int32_t H, int32_t B, const int32_t* h0,
                   const int32_t* env, int32_t S, float* s, float* s_next, float* a_out, float* r_out,
                   hipStream_t stream, int* rc);
// pmenv_replay_gather_seq: the window stores' cache-policy bits (< 0: the product's rule)
// and the elements per chunk (0: the product's rule)
void replay_seq_knobs(int* policy, int* chunk);
// pmenv_ind_*: the recurrences' form (ind_plan.h IndForm; < 0: the product's rule)
int ind_form();
bool rollout_gather(const float* series, int32_t T, int32_t N, int32_t F, int32_t W, const int32_t* start,
                    const float* weights, int32_t T_rec, int32_t B, int32_t ring_mode, const int32_t* t_idx,
                    const int32_t* env, int32_t S, float* s, hipStream_t stream, int* rc);
bool metrics(const double* returns, const double* values, const float* weights, int32_t T, int32_t B, int32_t N,
             double risk_free_rate, double periods, double* out, hipStream_t stream, int* rc);
bool batch_reward_forward(const float* a, const float* v_prev, const float* p, int32_t B, int32_t N,
                          int32_t reward_kind, int32_t norm, double scale, double* work, float* reward_out,
                          float* ret_out, hipStream_t stream, int* rc);
}  // namespace pmenv_tools
