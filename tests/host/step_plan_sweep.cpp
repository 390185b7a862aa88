// step_plan_sweep.cpp — the step's shape plan (pm-rl_amd/csrc/step_plan.h) from a plain host
// program: no HIP header, no device, no library. Reads one cfg per line from stdin,
//     B N W F commission path
// (path: a pmenv_step_path_kind; the other cfg fields as pmenv_cfg_default sets them) and
// prints what pmenv_step_path_for(cfg, path, 1) returns: an empty line for a cfg or a path
// that is refused. tests/test_step_plan_host.py compiles it with the host C++ compiler, once
// plainly and once under the address and undefined-behaviour sanitizers, and compares its
// output with the library's.
#include <string.h>

#include "../../pm-rl_amd/csrc/step_plan.h"

int main() {
    long long B, N, W, F;
    int path;
    double commission;
    char out[512];
    while (scanf("%lld %lld %lld %lld %lf %d", &B, &N, &W, &F, &commission, &path) == 6) {
        pmenv_cfg c;
        memset(&c, 0, sizeof(c));
        c.num_envs = (int32_t)B;
        c.num_assets = (int32_t)N;
        c.window = (int32_t)W;
        c.features = (int32_t)F;
        c.close_channel = F >= 5 ? 3 : 0;
        c.reward_kind = PMENV_REWARD_LOG_RETURN;
        c.norm_mode = PMENV_NORM_AND;
        c.ring_mode = PMENV_RING_STORAGE;
        c.ret_mode = PMENV_RET_GROSS;
        c.mu_max_iter = 100;
        c.init_cash = 25000.0;
        c.commission = commission;
        c.reward_scale = 1.0;
        c.risk_free_rate = 0.04;
        c.sharpe_eta = 0.01;
        c.mu_tol = 1e-10;
        pmenv_host::step_plan_path_for(c, path, true, out, sizeof(out));
        puts(out);
    }
    return 0;
}
