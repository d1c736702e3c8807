// path_statistics.hpp -- the exact score and the transition counts of GIVEN state paths (torbi_amd/paths.py, PATHS.md).
//
// A path q of item b (T int32 columns, F = the item's frames clamped to [1, T]) is scored by the decoder's alpha recurrence
// followed along the path, every sum float32 with one rounding (the build has -ffp-contract=off), A indexed [next][prev]:
//     s_0 = fl(o_0[q_0] + pi[q_0]);   s_t = fl(o_t[q_t] + fl(s_{t-1} + A[q_t][q_{t-1}]))   1 <= t < F;   score = s_{F-1}
// and counted as  X[q_t][q_{t-1}] += w (1 <= t < F),  I[q_0] += w,  in float64, rounded to float32 once at the end.  Only the
// cells on the path are read; NaN and +-inf propagate by plain IEEE arithmetic.  A path with an index outside [0, S) at a
// column t < F is void: score -inf, no counts.
//
// One wave per path, four waves per workgroup; the K paths of an item are neighbouring waves, so their gathers from the
// item's observation rows share L2 lines.  Pass 1 reads the columns t < F, 64 per step, and votes on void -- before anything
// is counted.  Pass 2 walks chunks of 64 frames: lane l owns frame base + l, takes q_{t-1} from its neighbour lane (lane 0
// from the chunk before), gathers its (o, a) pair and issues its count as one float64 atomic; then the wave walks the 64
// pairs in order, every lane holding the same running sum.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "scratch.hpp"

namespace ps {

constexpr int kWaves = 4;                 // paths per workgroup
constexpr int kThreads = 64 * kWaves;
constexpr int kMaxStates = 16384;         // (S * S float64 accumulators: 2 GiB there)

struct Layout {
    double *x, *i;                        // (S, S) and (S,) accumulators, zeroed by the call
    size_t zeroed;                        // bytes from x that the call zeroes (both regions and the gap between them)
    size_t total;
};

// `base`: the caller's workspace aligned up to 256 bytes, or null for the byte count alone.  Without counts: nothing.
inline Layout layout(char *base, int S, bool counts) {
    Layout l{};
    if (!counts) return l;
    Scratch a(base);
    l.x = a.take<double>((size_t)S * S);
    l.i = a.take<double>((size_t)S);
    l.zeroed = a.bytes;
    l.total = a.bytes + 256;              // (room to align the caller's base)
    return l;
}

__device__ __forceinline__ float lane_value(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// scores == null: counts only (observation, transition, initial unread); x == null: scores only (weights unread).
// transition == null: every entry is `uniform_value`.
__global__ __launch_bounds__(kThreads) void ps_kernel(const float *__restrict__ observation, const int32_t *__restrict__ batch_frames,
                                                      const float *__restrict__ transition, float uniform_value,
                                                      const float *__restrict__ initial, const int32_t *__restrict__ indices,
                                                      const float *__restrict__ weights, float *__restrict__ scores,
                                                      double *__restrict__ x, double *__restrict__ first, int B, int T, int S,
                                                      int K) {
    const int lane = threadIdx.x & 63;
    const size_t path = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (path >= (size_t)B * K) return;                              // (uniform over the wave)
    const size_t b = path / (size_t)K;
    int F = batch_frames[b];
    F = F < 1 ? 1 : (F > T ? T : F);
    const int32_t *__restrict__ q = indices + path * (size_t)T;

    // pass 1: void?
    bool outside = false;
    for (int base = 0; base < F; base += 64) {
        const int t = base + lane;
        if (t < F) outside |= (uint32_t)q[t] >= (uint32_t)S;
    }
    if (__ballot(outside) != 0) {
        if (scores && lane == 0) scores[path] = -INFINITY;
        return;
    }

    const bool scoring = scores != nullptr, counting = x != nullptr;
    const double w = counting ? (weights ? (double)weights[path] : 1.0) : 0.0;
    const float *__restrict__ rows = scoring ? observation + b * (size_t)T * S : nullptr;
    float s = 0.f;
    int carry = 0;                                                  // q_{base - 1}
    for (int base = 0; base < F; base += 64) {
        const int t = base + lane;
        const bool live = t < F;
        const int qt = live ? q[t] : 0;
        const int left = __shfl_up(qt, 1);
        const int qp = lane == 0 ? carry : left;
        carry = __builtin_amdgcn_readlane(qt, 63);
        float o = 0.f, a = 0.f;
        if (live) {
            if (scoring) {
                o = rows[(size_t)t * S + qt];
                a = t == 0 ? initial[qt] : (transition ? transition[(size_t)qt * S + qp] : uniform_value);
            }
            if (counting) {
                if (t == 0) atomicAdd(first + qt, w);
                else atomicAdd(x + (size_t)qt * S + qp, w);
            }
        }
        if (scoring) {
            const int n = F - base < 64 ? F - base : 64;            // (uniform)
            if (base == 0) s = lane_value(o, 0) + lane_value(a, 0);
            for (int l = base == 0 ? 1 : 0; l < n; ++l) s = lane_value(o, l) + (s + lane_value(a, l));
        }
    }
    if (scoring && lane == 0) scores[path] = s;
}

// the one rounding of the counts: float64 accumulators to the float32 outputs
__global__ __launch_bounds__(256) void ps_round_kernel(const double *__restrict__ x, const double *__restrict__ first,
                                                       float *__restrict__ x_out, float *__restrict__ first_out, int S) {
    const size_t cells = (size_t)S * S, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < cells + S; e += stride) {
        if (e < cells) x_out[e] = (float)x[e];
        else first_out[e - cells] = (float)first[e - cells];
    }
}

}  // namespace ps
