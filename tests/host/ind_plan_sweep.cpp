// ind_plan_sweep.cpp — the technical indicators' plan (pm-rl_amd/csrc/ind_plan.h) from a plain
// host program: no HIP header, no device, no library. Reads one request per line from stdin,
//     <kind> T N n_ops { op_kind p0 p1 p2 f0 f1 } x n_ops
// with <kind> L (pmenv_ind_layout: prints the status, K and the lookback), W (the workspace
// bytes) or P (pmenv_ind_path's string); L ignores T and N.
// tests/test_indicators_host.py compiles it with the host C++ compiler, once plainly and once
// under the address and undefined-behaviour sanitizers, and compares its output with the
// library's.
#include <vector>

#include "../../pm-rl_amd/csrc/ind_plan.h"

int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        long long T, N, n_ops;
        if (scanf("%lld %lld %lld", &T, &N, &n_ops) != 3 || n_ops < 0 || n_ops > 1000) return 2;
        std::vector<pmenv_ind_op> ops((size_t)n_ops);             // exactly n_ops: a read past them is caught
        for (auto& op : ops) {
            long long k, p0, p1, p2;
            if (scanf("%lld %lld %lld %lld %lf %lf", &k, &p0, &p1, &p2, &op.f[0], &op.f[1]) != 6) return 2;
            op.kind = (int32_t)k;
            op.p[0] = (int32_t)p0;
            op.p[1] = (int32_t)p1;
            op.p[2] = (int32_t)p2;
        }
        const pmenv_ind_op* ptr = ops.empty() ? nullptr : ops.data();
        if (kind == 'L') {
            int32_t K = -1, L = -1;
            const int rc = pmenv_host::ind_layout(ptr, (int32_t)n_ops, &K, &L);
            printf("%d %d %d\n", rc, (int)K, (int)L);
        } else if (kind == 'W') {
            const pmenv_host::IndPlan p = pmenv_host::ind_plan((int32_t)T, (int32_t)N, ptr, (int32_t)n_ops);
            printf("%zu\n", p.ok ? p.work_bytes : (size_t)0);
        } else if (kind == 'P') {
            char out[512];
            pmenv_host::ind_plan_describe(pmenv_host::ind_plan((int32_t)T, (int32_t)N, ptr, (int32_t)n_ops), out,
                                          sizeof(out));
            puts(out);
        } else {
            return 2;
        }
    }
    return 0;
}
