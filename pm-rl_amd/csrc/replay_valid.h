// replay_valid.h — the valid (start, env) pairs of a replay whose envs end their episodes on
// their own (include/pmenv.h, "per-env episodes"): replay/buffer.py:47-59 draws a start
// inside one epoch; with an episode id per (ring row, env) the question "do rows st ..
// st + need - 1 of env b share one episode" has H * B answers, kept as one bit each.
//
//   bits   [span][ceil(B / 64)] u64: bit b & 63 of word (st, b >> 6) is set iff
//          env_episode[(oldest + st) % H, b] == env_episode[(oldest + st + need - 1) % H, b]
//          (ids never decrease along the ring for one env: the first and the last row decide)
//   rowsum [span + 1] i64: rowsum[st] = the pairs of rows < st, rowsum[span] = the total
//
// valid_select then finds the k-th pair in (st ascending, env ascending) order: the row by
// bisection of rowsum, the word by a wave scan of the row's popcounts, the bit by a ballot.
// Integer arithmetic throughout: the map and a draw are the same bits whatever the dispatch.
#pragma once
#include "common.h"
#include "prio.h"

namespace pmenv_dev {

constexpr int kValidWordsPerWave = 4;      // words a wave has in flight (eight loads)

// One workgroup per start offset, a wave per 64 envs of it: two coalesced loads, one ballot,
// one word stored by lane 0. Wave w takes words w, w + waves, ..; kValidWordsPerWave of them
// a round, every load of the round issued before the first ballot. The waves' popcounts meet
// in LDS and thread 0 writes the row's count to rowsum[st + 1] (valid_scan_kernel turns the
// counts into prefix sums).
__global__ void __launch_bounds__(1024)
valid_bits_kernel(const int32_t* __restrict__ ep, int H, int B, int oldest, int need, int WB,
                  unsigned long long* __restrict__ bits, long long* __restrict__ rowsum) {
    __shared__ int part[16];
    const int st = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int32_t* __restrict__ first = ep + (size_t)((oldest + st) % H) * B;
    const int32_t* __restrict__ last = ep + (size_t)((oldest + st + need - 1) % H) * B;
    int cnt = 0;
    for (int w0 = w; w0 < WB; w0 += waves * kValidWordsPerWave) {
        int32_t x[kValidWordsPerWave], y[kValidWordsPerWave];
#pragma unroll
        for (int k = 0; k < kValidWordsPerWave; ++k) {
            const int e = (w0 + k * waves) * 64 + lane;
            const bool in = w0 + k * waves < WB && e < B;
            x[k] = in ? first[e] : 0;
            y[k] = in ? last[e] : 1;                       // past B: never equal, the padding bits stay 0
        }
#pragma unroll
        for (int k = 0; k < kValidWordsPerWave; ++k) {
            const int word = w0 + k * waves;               // wave-uniform
            const unsigned long long m = __ballot(x[k] == y[k]);
            if (word < WB) {
                if (lane == 0) bits[(size_t)st * WB + word] = m;
                cnt += __popcll(m);
            }
        }
    }
    if (lane == 0) part[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long tot = 0;
        for (int k = 0; k < waves; ++k) tot += part[k];
        rowsum[st + 1] = tot;
    }
}

// rowsum[0] = 0 and the counts of rowsum[1 .. span] become their inclusive prefix sums, in
// place, by one workgroup: 1,024 entries a round (a Hillis-Steele scan in LDS) on top of the
// rounds before. span = 0 writes rowsum[0] alone.
__global__ void __launch_bounds__(1024) valid_scan_kernel(long long* rowsum, int span) {
    __shared__ long long sh[2][1024];
    const int tid = threadIdx.x;
    long long carry = 0;
    if (tid == 0) rowsum[0] = 0;
    for (int i0 = 0; i0 < span; i0 += 1024) {
        const int i = i0 + tid;
        int cur = 0;
        sh[0][tid] = i < span ? rowsum[i + 1] : 0;
        __syncthreads();
#pragma unroll
        for (int d = 1; d < 1024; d <<= 1) {
            sh[cur ^ 1][tid] = sh[cur][tid] + (tid >= d ? sh[cur][tid - d] : 0);
            cur ^= 1;
            __syncthreads();
        }
        if (i < span) rowsum[i + 1] = carry + sh[cur][tid];
        carry += sh[cur][1023];
        __syncthreads();                                   // sh[0] is rewritten next round
    }
}

__device__ __forceinline__ unsigned long long lane_value_u64(unsigned long long v, int lane) {
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, lane);
    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// One wave per sample: k = clamp(floor(u * total), 0, total - 1), a NaN u counts as 0; the
// row st with rowsum[st] <= k < rowsum[st + 1] by bisection (at most ceil(log2(span + 1))
// steps); inside the row, 64 words a round: lane c holds word c's popcount, the wave scans
// them (prio.h's wave_scan; the counts are small integers, exact in f64), a ballot finds
// the first word whose inclusive prefix exceeds the residual, and the lanes of that word
// find its r-th set bit by one more ballot. total == 0 writes -1 to both outputs and reads
// no bits. A map that does not hold k pairs (a buffer valid_build never wrote) gives -1 too.
__global__ void __launch_bounds__(256)
valid_select_kernel(const unsigned long long* __restrict__ bits, const long long* __restrict__ rowsum, int H, int B,
                    int oldest, int span, const double* __restrict__ u, int S, int32_t* __restrict__ h0_out,
                    int32_t* __restrict__ env_out) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= S) return;                                    // uniform per wave
    const long long total = rowsum[span];
    if (total <= 0) {
        if (lane == 0) h0_out[j] = env_out[j] = -1;
        return;
    }
    const double x = floor(u[j] * (double)total);
    long long k = !(x >= 0.0) ? 0 : x >= (double)total ? total - 1 : (long long)x;
    k = k > total - 1 ? total - 1 : k;
    int lo = 0, hi = span;                                 // rowsum[lo] <= k < rowsum[hi]
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int mid = (lo + hi) >> 1;
        if (rowsum[mid] <= k) lo = mid;
        else hi = mid;
    }
    const int st = lo;
    const int WB = (B + 63) >> 6;
    double r = (double)(k - rowsum[st]);                   // the pair's rank inside its row
    int word = -1;
    unsigned long long m = 0;
    for (int w0 = 0; w0 < WB; w0 += 64) {
        const unsigned long long v = w0 + lane < WB ? bits[(size_t)st * WB + w0 + lane] : 0ull;
        const double incl = wave_scan((double)__popcll(v), lane);
        const unsigned long long hit = __ballot(incl > r);
        if (hit) {
            const int c = __ffsll((long long)hit) - 1;
            r -= c > 0 ? lane_value(incl, c - 1) : 0.0;
            m = lane_value_u64(v, c);
            word = w0 + c;
            break;                                         // uniform: hit is a ballot
        }
        r -= lane_value(incl, 63);
    }
    // the r-th set bit: the lane whose bit is set with exactly r set bits below it
    const int rank = (int)r;
    const bool me = word >= 0 && ((m >> lane) & 1ull) && __popcll(m & ((1ull << lane) - 1ull)) == rank;
    const unsigned long long pick = __ballot(me);
    if (lane == 0) {
        const bool ok = pick != 0ull;
        h0_out[j] = ok ? (oldest + st) % H : -1;
        env_out[j] = ok ? word * 64 + (__ffsll((long long)pick) - 1) : -1;
    }
}

}  // namespace pmenv_dev
