// prio.h — the resident priority tree of the device replay (include/pmenv.h, "prioritized
// sampling"): a radix-64 sum tree over the ring's one-step starts, f32 leaves and f64 nodes
// in one caller-owned buffer. Every node is recomputed from its 64 children by one wave in a
// fixed order (wave_sum), never updated by a delta: no floating-point atomics, and two waves
// that refresh the same node write the same bits.
#pragma once
#include <float.h>

#include "common.h"

namespace pmenv_dev {

constexpr int kPrioMaxLevels = 6;          // leaves < 2^31: at most 2^25, 2^19, 2^13, 2^7, 2 nodes
constexpr size_t kPrioHeaderBytes = 64;    // [0] f32: the running maximum leaf value

// Byte layout (include/pmenv.h): header, leaves, level 1 .. level `levels`; every level is
// padded with zeros to a multiple of 64 entries, so a wave's 64 loads are always in bounds
// and the padding adds nothing to a sum.
struct PrioTree {
    int levels;                            // internal levels, >= 1; the top one has <= 64 nodes
    int64_t n[kPrioMaxLevels + 1];         // n[0] = leaves, n[k] = ceil(n[k-1] / 64)
    size_t off[kPrioMaxLevels + 1];
    size_t bytes;
};

inline PrioTree prio_layout(int64_t leaves) {
    PrioTree t{};
    t.n[0] = leaves;
    t.off[0] = kPrioHeaderBytes;
    size_t off = kPrioHeaderBytes + (size_t)((leaves + 63) / 64 * 64) * sizeof(float);
    int64_t n = leaves;
    int k = 0;
    do {
        n = (n + 63) / 64;
        ++k;
        t.n[k] = n;
        t.off[k] = off;
        off += (size_t)((n + 63) / 64 * 64) * sizeof(double);
    } while (n > 64);
    t.levels = k;
    t.bytes = off;
    return t;
}

// max((|td| + eps)^alpha, FLT_MIN) in f64, rounded once (and kept finite); a non-finite td
// takes the current maximum
__device__ __forceinline__ float prio_value(float td, double alpha, double eps, float cur_max) {
    if (!isfinite(td)) return cur_max;
    const double v = pow((double)fabsf(td) + eps, alpha);
    return (float)fmin(fmax(v, (double)FLT_MIN), (double)FLT_MAX);
}

// inclusive prefix sums over the wave's 64 lanes: four DPP row shifts scan each 16-lane
// row, the three row totals come from v_readlane and are added in a fixed order
__device__ __forceinline__ double wave_scan(double v, int lane) {
    v += dpp_shift<kRowShr1>(v, 0.0);
    v += dpp_shift<kRowShr2>(v, 0.0);
    v += dpp_shift<kRowShr4>(v, 0.0);
    v += dpp_shift<kRowShr8>(v, 0.0);
    const double t0 = lane_value(v, 15), t1 = lane_value(v, 31), t2 = lane_value(v, 47);
    const int row = lane >> 4;
    const double before = row == 0 ? 0.0 : row == 1 ? t0 : row == 2 ? t0 + t1 : (t0 + t1) + t2;
    return v + before;
}

__global__ void __launch_bounds__(256) prio_init_kernel(unsigned long long* words, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        words[i] = i == 0 ? 0x3F800000ull : 0ull;          // header: maximum = 1.0f
}

// One wave per touched node of level k (shift = 6k). Level 1 also writes the leaves: a lane
// whose leaf lies in the close range stores 0, in the open range the maximum. Every wave
// applies both ranges, so two waves that meet in one node (small n) write the same bits.
// children: the leaves (k = 1) or level k - 1. ep_first / ep_last [n] (pmenv_prio_fill_env, level 1 only;
// nullptr: no mask): leaf o0 + i opens only where ep_first[i] == ep_last[i], the envs whose
// window lies in one episode; the others keep the 0 their row's close left.
__global__ void __launch_bounds__(256)
prio_fill_kernel(const float* hdr, float* leaves, const double* children, double* nodes, int64_t leaf_count,
                 int64_t c0, int64_t o0, int64_t n, int shift, const int32_t* ep_first, const int32_t* ep_last) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t cf = c0 >> shift, cc = c0 < 0 ? 0 : ((c0 + n - 1) >> shift) - cf + 1;
    const int64_t of = o0 >> shift, oc = o0 < 0 ? 0 : ((o0 + n - 1) >> shift) - of + 1;
    if (w >= cc + oc) return;
    const int64_t node = w < cc ? cf + w : of + (w - cc);
    const int64_t i = node * 64 + lane;
    double v;
    if (shift == 6) {
        float x = leaves[i];                               // padded: in bounds
        if (i < leaf_count) {
            if (c0 >= 0 && i >= c0 && i < c0 + n) leaves[i] = x = 0.0f;
            if (o0 >= 0 && i >= o0 && i < o0 + n && (!ep_first || ep_first[i - o0] == ep_last[i - o0]))
                leaves[i] = x = hdr[0];
        }
        v = (double)x;
    } else {
        v = children[i];
    }
    v = wave_sum(v);
    if (lane == 0) nodes[node] = v;
}

// update, pass 1: every live touched leaf takes the smallest positive bit pattern, so that
// pass 2's integer max sees the new values alone (the old value is no candidate)
__global__ void __launch_bounds__(256)
prio_mark_kernel(uint32_t* leaf_bits, int64_t leaf_count, const int32_t* leaf, int S) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= S) return;
    const int32_t i = leaf[j];
    if (i < 0 || i >= leaf_count) return;
    if (leaf_bits[i] != 0u) leaf_bits[i] = 1u;
}

// update, pass 2: non-negative floats order as their bit patterns: an integer atomicMax
__global__ void __launch_bounds__(256)
prio_apply_kernel(const float* hdr, uint32_t* leaf_bits, int64_t leaf_count, const int32_t* leaf, const float* td,
                  int S, double alpha, double eps) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= S) return;
    const int32_t i = leaf[j];
    if (i < 0 || i >= leaf_count) return;
    if (leaf_bits[i] == 0u) return;                        // closed or overwritten since it was sampled
    atomicMax(&leaf_bits[i], __float_as_uint(prio_value(td[j], alpha, eps, hdr[0])));
}

// update, pass 3 .. : one wave per sample refreshes its leaf's ancestor of level k; the
// level-1 launch also raises the header's maximum to the finite new values (an integer
// atomicMax again; no value this launch writes depends on what it reads from the header)
__global__ void __launch_bounds__(256)
prio_refresh_kernel(uint32_t* hdr_bits, const float* leaves, const double* children, double* nodes,
                    int64_t leaf_count, const int32_t* leaf, const float* td, int S, double alpha, double eps,
                    int shift) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= S) return;
    const int32_t l = leaf[j];
    if (l < 0 || l >= leaf_count) return;
    if (shift == 6 && lane == 0 && isfinite(td[j])) {
        // the header only grows, so a plain read decides whether the atomic is needed at all
        // (8,192 atomics on one word cost 80 us; the result is the same maximum either way)
        const uint32_t v = __float_as_uint(prio_value(td[j], alpha, eps, 0.0f));
        if (v > *(volatile uint32_t*)hdr_bits) atomicMax(hdr_bits, v);
    }
    if (leaves[l] == 0.0f) return;                         // untouched: its ancestors keep their bits
    const int64_t node = (int64_t)l >> shift;
    const int64_t i = node * 64 + lane;
    double v = shift == 6 ? (double)leaves[i] : children[i];
    v = wave_sum(v);
    if (lane == 0) nodes[node] = v;
}

// One wave per sample. Lane c loads child c of the current node (one coalesced 512-B or
// 256-B run), the wave scans the 64 values, a ballot finds the first positive child whose
// inclusive prefix exceeds the residual, and v_readlane moves that child's exclusive prefix
// out. The top level (<= 64 nodes, padded to 64) is scanned as the children of a virtual
// root; its last prefix is `total`. Writes the leaf's value to p_out (prio_weight_kernel
// turns it into the weight). An empty tree gives leaf 0 and value 0.
__global__ void __launch_bounds__(256)
prio_sample_kernel(const char* tree, PrioTree t, int32_t B, const double* u, int S, int32_t* leaf_out,
                   int32_t* h0_out, int32_t* env_out, float* p_out) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= S) return;
    int64_t node = 0;
    double r = 0.0, p = 0.0;
    bool empty = false;
#pragma unroll
    for (int k = kPrioMaxLevels + 1; k >= 1; --k) {
        if (k > t.levels + 1 || empty) continue;
        const int64_t i = node * 64 + lane;
        const double v = k == 1 ? (double)reinterpret_cast<const float*>(tree + t.off[0])[i]
                                : reinterpret_cast<const double*>(tree + t.off[k - 1])[i];
        const double incl = wave_scan(v, lane);
        if (k == t.levels + 1) {
            double x = u[j];
            x = x >= 0.0 ? x : 0.0;                        // a NaN or negative u: the first leaf
            r = x * lane_value(incl, 63);
        }
        const unsigned long long pos = __ballot(v > 0.0);
        const unsigned long long hit = __ballot(v > 0.0 && incl > r);
        if (pos == 0ull) {
            empty = true;
            continue;
        }
        // rounding may leave the residual at or above the node's sum: the last positive child
        const int c = hit ? __ffsll((long long)hit) - 1 : 63 - __clzll((long long)pos);
        const double excl = lane_value(incl, c > 0 ? c - 1 : 0);
        r = fmax(r - (c > 0 ? excl : 0.0), 0.0);
        p = lane_value(v, c);
        node = node * 64 + c;
        if (node >= t.n[k - 1]) node = t.n[k - 1] - 1;     // only a buffer that pmenv_prio_init never saw
    }
    if (lane == 0) {
        const int32_t l = empty ? 0 : (int32_t)node;
        leaf_out[j] = l;
        h0_out[j] = l / B;
        env_out[j] = l % B;
        p_out[j] = empty ? 0.0f : (float)p;
    }
}

// weight_j = (p_j / min_k p_k)^(-beta) in f64, rounded once. Up to 16 workgroups: each takes
// the batch minimum for itself from the tree's leaves (which this call never writes; p_out
// is being overwritten by the other workgroups), then turns its own share of p_out into
// weights. The minimum is order-free.
__global__ void __launch_bounds__(1024)
prio_weight_kernel(const float* leaves, const int32_t* leaf, float* w, int S, double beta) {
    __shared__ double part[16];
    double m = INFINITY;
    for (int i = threadIdx.x; i < S; i += 1024) {
        const float p = leaves[leaf[i]];
        if (p > 0.0f) m = fmin(m, (double)p);
    }
    m = wave_min(m);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    m = part[0];
    for (int k = 1; k < 16; ++k) m = fmin(m, part[k]);
    for (int i = blockIdx.x * 1024 + threadIdx.x; i < S; i += gridDim.x * 1024) {
        const float p = w[i];
        w[i] = p > 0.0f ? (float)pow((double)p / m, -beta) : 0.0f;
    }
}

}  // namespace pmenv_dev
