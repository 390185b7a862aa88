// episode.h — per-env episodes on a resident market series (pmenv_restart_days).
//
// Lockstep envs that start on different days of one series end on different steps. After
// every resident-series step the caller asks, per env, whether the bar just appended was the
// env's last; the envs that ended are put back at their restart day: window, weight channel
// and state as pmenv_window_init_days followed by pmenv_reset(obs, mask) leave them. The work
// is proportional to the envs that restart, not to B: a workgroup owns a slice of 64
// consecutive envs, wave 0 decides them (one lane per env) and ballots the slice's restart
// mask, and a workgroup whose mask is zero exits after three coalesced loads and two stores.
#pragma once
#include "common.h"

namespace pmenv_dev {

constexpr int kEpSlice = 64;      // envs per workgroup: one lane of wave 0 each
constexpr int kEpBlock = 256;
// the workgroup's LDS: 16 bytes for the slice's mask, then (staged form) the env's series slab;
// kept within the 64 KiB every launch may ask for without raising the kernel's limit
constexpr size_t kEpMaskBytes = 16;
constexpr size_t kEpLdsMax = 64 * 1024;

// STAGED: F = 5, 16-B aligned series / window / ring, env windows of whole 16-B chunks, and the
// W days' [W, N, 4] slab within LDS — the W days restart .. restart + W - 1 are one contiguous
// run of the series, staged with coalesced 16-B loads, and the [N, W, 5] window is written as
// 16-B chunks composed from LDS (rollout_gather_tile_kernel's form, replay.h). Plain stores:
// the next step reads the window at once. Otherwise dword loads and stores per (n, t) row,
// as window_init_days_kernel and reset_kernel. Both forms write the same bytes.
template <bool STAGED>
static __global__ __launch_bounds__(kEpBlock) void restart_days_kernel(StepParams p, float* obs, const float* series,
                                                                       int T, int32_t* day, const int32_t* end,
                                                                       const int32_t* restart, uint8_t* done) {
    extern __shared__ __attribute__((aligned(16))) float ep_sh[];
    unsigned long long* sh_mask = reinterpret_cast<unsigned long long*>(ep_sh);
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * kEpSlice;
    const int N = p.N, W = p.W, F = p.F;
    if (tid < kEpSlice) {
        const int b = b0 + tid;
        bool rs = false;
        if (b < p.B) {
            const int32_t next = day[b] + 1, e = end[b], r = restart[b];
            rs = next >= e;
            day[b] = rs ? r + W : next;
            done[b] = rs ? 1 : 0;
        }
        const unsigned long long m = __ballot(rs);
        if (tid == 0) *sh_mask = m;
    }
    __syncthreads();
    // the mask is the same in every thread: keep it in scalar registers, so the loop over its
    // set bits (and the barriers inside) is uniform across the workgroup
    const unsigned long long mv = *sh_mask;
    unsigned long long m =
        ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(mv >> 32)) << 32) |
        (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)mv);
    while (m) {
        const int b = b0 + __builtin_ctzll(m);
        m &= m - 1;
        const int r0 = __builtin_amdgcn_readfirstlane(restart[b]);
        float* ob = obs + (size_t)b * N * W * F;
        if (tid == 0) {                                // reset_kernel's scalars
            p.value[b] = p.init_cash;
            p.k[b] = 0;
            p.sa[b] = 0.0;
            p.sb[b] = 0.0;
        }
        for (int n = tid; n < N; n += kEpBlock) p.w_new[(size_t)b * N + n] = n == 0 ? 1.0f : 0.0f;
        float* ringb = p.ring + (size_t)b * W * N;     // e0 in slot 0
        if constexpr (STAGED) {
            constexpr int Fs = 5;
            f4* slab4 = reinterpret_cast<f4*>(ep_sh + kEpMaskBytes / 4);
            const float* slab = ep_sh + kEpMaskBytes / 4;
            const int nd = W * N;                      // one f4 per (day, asset)
            // days outside the series read NaN; a negative restart day gives a NaN window
            // (window_init_days_kernel's rule)
            const int64_t in_days = r0 >= 0 ? (int64_t)T - r0 : 0;
            const int nv = (int)(in_days <= 0 ? 0 : (in_days >= W ? nd : in_days * N));
            const f4* src = reinterpret_cast<const f4*>(series) + (int64_t)(r0 >= 0 ? r0 : 0) * N;
            for (int i0 = 0; i0 < nd; i0 += 4 * kEpBlock) {   // a round's loads in flight before its LDS writes
                f4 v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = i0 + k * kEpBlock + tid;
                    v[k] = f4{NAN, NAN, NAN, NAN};
                    if (i < nv) v[k] = src[i];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = i0 + k * kEpBlock + tid;
                    if (i < nd) slab4[i] = v[k];
                }
            }
            f4* ring4 = reinterpret_cast<f4*>(ringb);  // W * N is a multiple of 4 here
            for (int i = tid; i < nd / 4; i += kEpBlock) ring4[i] = f4{i == 0 ? 1.0f : 0.0f, 0.0f, 0.0f, 0.0f};
            __syncthreads();
            const int WF = W * Fs;
            const int nq = N * WF / 4;
            f4* out = reinterpret_cast<f4*>(ob);
            for (int q = tid; q < nq; q += kEpBlock) {
                const int e = 4 * q;
                int n = (int)fdiv((uint32_t)e, p.div_wf);
                const int rem = e - n * WF;
                int t = (int)fdiv((uint32_t)rem, p.div_f);
                int f = rem - t * Fs;
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    // channel 4: the seed of the weight channel, 1 at (n = 0, t = W - 1)
                    v[k] = f < Fs - 1 ? slab[(t * N + n) * 4 + f] : ((n == 0 && t == W - 1) ? 1.0f : 0.0f);
                    if (++f == Fs) {
                        f = 0;
                        if (++t == W) {
                            t = 0;
                            ++n;
                        }
                    }
                }
                out[q] = f4{v[0], v[1], v[2], v[3]};
            }
            for (int n = tid; n < N; n += kEpBlock)
                p.last_close[(size_t)b * N + n] = slab[((W - 1) * N + n) * 4 + p.close_ch];
            __syncthreads();                           // the slab is restaged for the next env
        } else {
            const int Fm = F - 1;
            for (int i = tid; i < W * N; i += kEpBlock) ringb[i] = i == 0 ? 1.0f : 0.0f;
            for (int i = tid; i < N * W; i += kEpBlock) {
                const int n = (int)fdiv((uint32_t)i, p.div_w);
                const int t = i - n * W;
                const int64_t d = (int64_t)r0 + t;
                const bool ok = r0 >= 0 && d < T;
                float* o = ob + (size_t)i * F;
                for (int f = 0; f < Fm; ++f) o[f] = ok ? series[((size_t)d * N + n) * Fm + f] : NAN;
                o[Fm] = (n == 0 && t == W - 1) ? 1.0f : 0.0f;
            }
            const int64_t dl = (int64_t)r0 + W - 1;    // the close row of the window's last day
            const bool okl = r0 >= 0 && dl < T;
            for (int n = tid; n < N; n += kEpBlock)
                p.last_close[(size_t)b * N + n] = okl ? series[((size_t)dl * N + n) * Fm + p.close_ch] : NAN;
        }
    }
}

}  // namespace pmenv_dev
