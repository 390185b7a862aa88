// ffd_plan_sweep.cpp — the fractional-differencing plan (pm-rl_amd/csrc/ffd_plan.h) from a
// plain host program: no HIP header, no device, no library. Reads one request per line from
// stdin,
//     W d thres T         the taps of order d: prints the status, the width and the taps' bits
//     P T C max_width     the apply kernel's name and geometry (pmenv_ffd_path's string)
//     S T C               the scalers' chunk count and workspace bytes
// tests/test_ffd_plan_host.py compiles it with the host C++ compiler, once plainly and once
// under the address and undefined-behaviour sanitizers, and compares its output with the
// library's.
#include <string.h>

#include <vector>

#include "../../pm-rl_amd/csrc/ffd_plan.h"

int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'W') {
            double d, thres;
            long long T;
            if (scanf("%lf %lf %lld", &d, &thres, &T) != 3) return 2;
            int32_t width = -1;
            int rc = pmenv_host::ffd_weights(d, thres, (int32_t)T, nullptr, 0, &width);
            std::vector<float> taps(rc == PMENV_OK && width > 0 ? (size_t)width : 0);   // exactly width: a write past it is caught
            if (rc == PMENV_OK && width > 0)
                rc = pmenv_host::ffd_weights(d, thres, (int32_t)T, taps.data(), width, &width);
            printf("%d %d", rc, (int)width);
            for (float t : taps) {
                uint32_t bits;
                memcpy(&bits, &t, sizeof(bits));
                printf(" %08x", bits);
            }
            puts("");
        } else if (kind == 'P') {
            long long T, C, mw;
            char out[160];
            if (scanf("%lld %lld %lld", &T, &C, &mw) != 3) return 2;
            pmenv_host::ffd_plan_describe(pmenv_host::ffd_plan((int32_t)T, (int32_t)C, (int32_t)mw), out, sizeof(out));
            puts(out);
        } else if (kind == 'S') {
            long long T, C;
            if (scanf("%lld %lld", &T, &C) != 2) return 2;
            printf("%lld %zu\n", (long long)pmenv_host::scale_chunks((int32_t)T, (int32_t)C),
                   pmenv_host::scale_workspace((int32_t)T, (int32_t)C));
        } else {
            return 2;
        }
    }
    return 0;
}
