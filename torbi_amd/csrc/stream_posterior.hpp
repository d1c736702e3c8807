// stream_posterior.hpp -- online filtering and fixed-lag smoothing: the forward-backward recurrence of forward_backward.hpp
// on frames that arrive in pieces (torbi_hip_stream_posterior_*, torbi_amd/stream_posterior.py, STREAM.md "Streaming
// posteriors").  The sum-product twin of stream.hpp: the same Info, the same ring addressing, the same tile rule.
//
// A stream holds n frames, the first `base` of them returned.  A push of f >= 1 frames returns gamma_{t|n'} (n' = n + f) for
// t = base .. n' - 1 - lag: row t of the whole-sequence posteriors of the stream's first n' frames.
//
// Per stream the caller owns (torbi_hip_stream_posterior_state_size; 4-byte words, packed, no initialisation):
//     L     [B][2]      words   the fp64 running sum of log c_t + m_t (low word first: the state is only 4-byte aligned)
//     a     [B][cap][S] fp32    a_t of the pending frames; frame `base + r` lives in slot (base_slot + r) % cap
//     e     [B][cap][S] fp32    e_t = exp(o_t - m_t) (frame 0: exp(initial + o_0 - m_0))
//     c     [B][cap]    fp32    c_t = sum_j a_t[j]
//     m     [B][cap]    fp32    m_t (kept for the caller; no kernel reads it back)
// The newest frame's a and c are the carried row of the next push, so they stay readable in their slot after the frame
// has been returned (slot base_slot - 1 when nothing is pending; a push loads them before it writes anything).
//
// E = exp(A) and its transpose are NOT built here: the caller passes both (torbi_amd/stream_posterior.py builds them once
// per decoder with torch.exp from a private copy of the matrix).
//
// A push is two launches, a flush the second alone:
//   sp_forward_kernel<G, J>   the scaled recurrence over every frame of the push in one launch; G streams per workgroup
//                             share each load of E^T ([prev][next], coalesced over next states, J = 4 consecutive states
//                             per thread with one 16-byte load per matrix row piece); the G previous rows double-buffered
//                             in LDS; one fma per cell
//   sp_backward_kernel<G, J>  one sweep from frame n' - 1 down to base, pending + f steps, reading E ([next][prev],
//                             coalesced over prev states); the w rows double-buffered in LDS; only the rows that leave
//                             are written.  A stream that returns nothing takes no step.
//
// A stream's bits depend on its own data and (t, n') only -- not on G, J, the ring slot, the cut into pushes or its
// neighbours: every cell sum runs over the previous states 0 .. S-1 in order as one fmaf chain per state; c_t is read back
// from the LDS row by thread tid as states tid, tid + 256, ... in order, a 64-lane butterfly per wave, then the 4 wave sums
// in order; the row maximum is order-free (NaN propagates through a flag); L is one fp64 add per frame.
// Vector stores only, no float atomics, nothing waits across workgroups, no host synchronisation.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "stream.hpp"

namespace stream_posterior {

using stream::Info;
using stream::slot_of;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxGroup = 16;
constexpr int kMaxLdsBytes = 64 * 1024;
// rows [2][G][S] fp32 of dynamic LDS beside 3 * kMaxGroup * kWaves words of wave partials: G = 1 fits up to here
constexpr int kMaxStates = 8000;

inline size_t lds_bytes(int G, int S) { return (size_t)2 * G * S * sizeof(float); }
inline bool fits(int G, int S) { return lds_bytes(G, S) + 3 * kMaxGroup * kWaves * 4 <= (size_t)kMaxLdsBytes; }

// rows a call returns for a stream that fits: push (frames >= 1) pending + frames - lag, flush (flagged) every pending row
__device__ __forceinline__ int leaving(const Info &in, int add, int lag) {
    const int n = in.pending + add - lag;
    return n > 0 ? n : 0;
}

// THE predicate of a call, applied to info[b] by both kernels.  Push (Tc >= 0): `frames` new rows (0 .. Tc) go into a ring
// of `cap` slots that holds `pending` rows, and the rows that leave fit the output; a fresh stream has nothing pending.
// Flush (Tc < 0): every pending row leaves.  A stream that fails keeps its state and its output rows untouched.
__device__ __forceinline__ bool call_fits(const Info &in, int Tc, int cap, int out_cap, int lag) {
    if (in.pending < 0 || in.base_slot < 0 || in.base_slot >= cap || in.pending > cap) return false;
    if (in.fresh != 0 && in.pending != 0) return false;
    if (Tc < 0) return in.pending <= out_cap;
    if (in.frames < 0 || in.frames > Tc || in.frames > cap - in.pending) return false;
    return in.frames == 0 || leaving(in, in.frames, lag) <= out_cap;
}

// frames a push appends to a stream: info's count, 0 for a stream whose info does not fit
__device__ __forceinline__ int new_frames(const Info &in, int Tc, int cap, int out_cap, int lag) {
    return call_fits(in, Tc, cap, out_cap, lag) ? in.frames : 0;
}

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

__device__ __forceinline__ double load_sum(const int32_t *w) { return __hiloint2double(w[1], w[0]); }
__device__ __forceinline__ void store_sum(int32_t *w, double v) { w[0] = __double2loint(v); w[1] = __double2hiint(v); }

template <int J>
__device__ __forceinline__ void load_piece(const float *__restrict__ p, float (&tr)[J]) {
    if constexpr (J == 4) {
        const float4 v = *reinterpret_cast<const float4 *>(p);
        tr[0] = v.x; tr[1] = v.y; tr[2] = v.z; tr[3] = v.w;
    } else {
        tr[0] = p[0];
    }
}

// acc[g][q] = sum_{i < S} mat[i][j0 + q] * row_g[i], i in order, one fmaf per cell; mat rows are S long.  The matrix pieces
// of the next U rows are requested before the cells of the current U are summed (U = 4 up to 8 streams; 16 streams have no
// registers to spare and take them one at a time): left to itself the compiler waits for every piece before it asks
// for the next one.  The order of the sums is the same either way.
template <int G, int J>
__device__ __forceinline__ void cell_sums(const float *__restrict__ mat, const float *rows, int S, int j0, float (&acc)[G][J]) {
    constexpr int U = G >= 16 ? 1 : 4;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int q = 0; q < J; ++q) acc[g][q] = 0.f;
    const int full = S - S % U;
    float ahead[U][J];
#pragma unroll
    for (int u = 0; u < U; ++u) load_piece<J>(mat + (size_t)(u < S ? u : S - 1) * S + j0, ahead[u]);
    for (int i = 0; i < full; i += U) {
        float tr[U][J];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int q = 0; q < J; ++q) tr[u][q] = ahead[u][q];
            const int r = i + U + u;                             // (past the end: the last row again, never used)
            load_piece<J>(mat + (size_t)(r < S ? r : S - 1) * S + j0, ahead[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float p = rows[(size_t)g * S + i + u];
#pragma unroll
                for (int q = 0; q < J; ++q) acc[g][q] = fmaf(tr[u][q], p, acc[g][q]);
            }
    }
    for (int i = full; i < S; ++i) {                            // ahead[i - full] holds row i
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u != i - full) continue;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float p = rows[(size_t)g * S + i];
#pragma unroll
                for (int q = 0; q < J; ++q) acc[g][q] = fmaf(ahead[u][q], p, acc[g][q]);
            }
        }
    }
}

// ---- forward: G streams of a tile, `frames` new rows each.  obs (B, Tc, S); et = E transposed ([prev][next]).
// Dynamic LDS: 2 * G * S floats.
template <int G, int J>
__global__ __launch_bounds__(kThreads) void sp_forward_kernel(const float *__restrict__ obs, int Tc, const Info *__restrict__ info,
                                                              const float *__restrict__ et, const float *__restrict__ initial,
                                                              int32_t *__restrict__ Lw, float *__restrict__ ring_a,
                                                              float *__restrict__ ring_e, float *__restrict__ ring_c,
                                                              float *__restrict__ ring_m, int cap, int out_cap, int lag, int B, int S) {
    extern __shared__ float rows[];          // [2][G][S]
    __shared__ float part_max[G][kWaves], part_sum[G][kWaves];
    __shared__ int part_nan[G][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * G;
    int fr[G], tmax = 0;
    Info in[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        in[g] = b0 + g < B ? info[b0 + g] : Info{0, 0, 0, 0};
        fr[g] = b0 + g < B ? new_frames(in[g], Tc, cap, out_cap, lag) : 0;
        tmax = max(tmax, fr[g]);
    }
    if (tmax == 0) return;
    // the carried rows and their sums
    float cprev[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const bool carry = fr[g] > 0 && !in[g].fresh;
        const size_t at = (size_t)(b0 + g) * cap + (carry ? slot_of(in[g].base_slot, in[g].pending - 1, cap) : 0);
        for (int i = tid; i < S; i += kThreads) rows[(size_t)g * S + i] = carry ? ring_a[at * S + i] : 0.f;
        cprev[g] = carry ? ring_c[at] : 1.f;
    }
    double L = 0.;                           // thread g carries the running sum of stream g
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (tid == g && fr[g] > 0 && !in[g].fresh) L = load_sum(Lw + 2 * (size_t)(b0 + g));
    __syncthreads();
    for (int t = 0; t < tmax; ++t) {
        const float *cur = rows + (size_t)(t & 1) * G * S;
        float *nxt = rows + (size_t)((t + 1) & 1) * G * S;
        // m_t: the NaN-propagating maximum of the frame's row (initial added on a stream's first frame), -inf read as 0
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (t >= fr[g]) continue;
            const float *o = obs + ((size_t)(b0 + g) * Tc + t) * S;
            const bool first = in[g].fresh && t == 0;
            float best = -INFINITY;
            int nan = 0;
            for (int i = tid; i < S; i += kThreads) {
                const float x = first ? initial[i] + o[i] : o[i];
                nan |= x != x;
                best = __builtin_fmaxf(best, x);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                best = __builtin_fmaxf(best, __shfl_xor(best, off, 64));
                nan |= __shfl_xor(nan, off, 64);
            }
            if (lane == 0) { part_max[g][wave] = best; part_nan[g][wave] = nan; }
        }
        __syncthreads();
        float mt[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float best = part_max[g][0];
            int nan = part_nan[g][0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) { best = __builtin_fmaxf(best, part_max[g][w]); nan |= part_nan[g][w]; }
            mt[g] = nan ? __builtin_nanf("") : (best == -INFINITY ? 0.f : best);
        }
        // a_t = e_t * (E a_{t-1}) / c_{t-1}
        for (int j0 = tid * J; j0 < S; j0 += kThreads * J) {
            float acc[G][J];
            cell_sums<G, J>(et, cur, S, j0, acc);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t >= fr[g]) continue;
                const size_t at = ((size_t)(b0 + g) * cap + slot_of(in[g].base_slot, in[g].pending + t, cap)) * S;
                const float *o = obs + ((size_t)(b0 + g) * Tc + t) * S;
                const bool first = in[g].fresh && t == 0;
#pragma unroll
                for (int q = 0; q < J; ++q) {
                    const int j = j0 + q;
                    const float e = expf((first ? initial[j] + o[j] : o[j]) - mt[g]);
                    float v = e;
                    if (!first) {
                        const float u = e * acc[g][q];
                        v = cprev[g] == 0.f ? u * 0.f : u / cprev[g];      // (after a zero-probability frame: 0, or NaN from NaN)
                    }
                    nxt[(size_t)g * S + j] = v;
                    ring_a[at + j] = v;
                    ring_e[at + j] = e;
                }
            }
        }
        __syncthreads();
        // c_t, in the one order that does not depend on G or J
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (t >= fr[g]) continue;
            float s = 0.f;
            for (int i = tid; i < S; i += kThreads) s += nxt[(size_t)g * S + i];
            s = wave_sum(s);
            if (lane == 0) part_sum[g][wave] = s;
        }
        __syncthreads();
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (t >= fr[g]) continue;
            float c = part_sum[g][0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) c += part_sum[g][w];
            cprev[g] = c;
            if (tid == g) {
                const size_t at = (size_t)(b0 + g) * cap + slot_of(in[g].base_slot, in[g].pending + t, cap);
                ring_c[at] = c;
                ring_m[at] = mt[g];
                L += log((double)c) + (double)mt[g];
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (tid == g && fr[g] > 0) store_sum(Lw + 2 * (size_t)(b0 + g), L);
}

// ---- backward: G streams of a tile, one sweep from the newest frame down to the first pending one.  ex = E ([next][prev]).
// Tc >= 0: the second launch of a push (the forward has appended info.frames rows); Tc < 0: a flush (info.frames = 1 flags
// the stream).  out [B][out_cap][S]: rows 0 .. count - 1 are the stream's frames base .. base + count - 1; counts (may be
// null) [B] = count, -1 where the info does not fit.  NaN rows where the stream's running sum is not finite.
// Dynamic LDS: 2 * G * S floats.
template <int G, int J>
__global__ __launch_bounds__(kThreads) void sp_backward_kernel(const Info *__restrict__ info, int Tc, const float *__restrict__ ex,
                                                               const int32_t *__restrict__ Lw, const float *__restrict__ ring_a,
                                                               const float *__restrict__ ring_e, const float *__restrict__ ring_c,
                                                               int cap, float *__restrict__ out, int out_cap,
                                                               int32_t *__restrict__ counts, int lag, int B, int S) {
    extern __shared__ float rows[];          // [2][G][S]: w of the step before, w of this step
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * G;
    const bool flush = Tc < 0;
    int P[G], count[G], kmax = 0;
    bool bad[G];
    Info in[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const bool here = b0 + g < B;
        in[g] = here ? info[b0 + g] : Info{0, 0, 0, 0};
        const bool ok = here && call_fits(in[g], Tc, cap, out_cap, lag);
        const bool asked = ok && in[g].frames != 0;
        P[g] = asked ? in[g].pending + (flush ? 0 : in[g].frames) : 0;
        count[g] = asked ? (flush ? in[g].pending : leaving(in[g], in[g].frames, lag)) : 0;
        if (count[g] == 0) P[g] = 0;                                 // nothing leaves: no step
        if (here && counts && tid == 0) counts[b0 + g] = ok ? count[g] : -1;
        kmax = max(kmax, P[g]);
        bad[g] = false;
        if (P[g] > 0) {
            const double L = load_sum(Lw + 2 * (size_t)(b0 + g));
            bad[g] = !(L == L) || L == (double)INFINITY || L == -(double)INFINITY;
        }
    }
    for (int k = 0; k < kmax; ++k) {
        const float *prev = rows + (size_t)(k & 1) * G * S;
        float *cur = rows + (size_t)((k + 1) & 1) * G * S;
        for (int i0 = tid * J; i0 < S; i0 += kThreads * J) {
            float acc[G][J];
            if (k > 0) cell_sums<G, J>(ex, prev, S, i0, acc);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (k >= P[g]) continue;
                const int r = P[g] - 1 - k;                          // the frame of this step, relative to base
                const size_t row = (size_t)(b0 + g) * cap + slot_of(in[g].base_slot, r, cap);
                const float c = ring_c[row];
#pragma unroll
                for (int q = 0; q < J; ++q) {
                    const int i = i0 + q;
                    const float beta = k == 0 ? 1.f : acc[g][q];
                    cur[(size_t)g * S + i] = (ring_e[row * S + i] * beta) / c;
                    if (r < count[g])
                        out[((size_t)(b0 + g) * out_cap + r) * S + i] = bad[g] ? __builtin_nanf("") : (ring_a[row * S + i] * beta) / c;
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace stream_posterior
