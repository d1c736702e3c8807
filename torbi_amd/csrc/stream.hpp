// stream.hpp -- exact streaming Viterbi: pushes of frames, incremental commits (torbi_hip_stream_*, torbi_amd/stream.py).
//
// Per stream the caller owns (torbi_hip_stream_state_bytes):
//     ring  [B][cap][S] fp32   posterior rows of the pending frames; frame `base + r` lives in slot (base_slot + r) % cap
//     memo  [B][cap]    int32  size of the survivor set a frontier walk found at that frame (0 = never walked)
//     bp    [B][S]      int32  scratch: backpointers of every state at the newest frame (first walk step)
// The newest row (the "carried" row) is the only state the recurrence needs; the pending rows are what the frontier walk
// and the backtrace recompute backpointers from.
//
// A push is three launches:
//   stream_forward_kernel   value-only recurrence over every frame of the push, one launch, G streams per workgroup sharing
//                           the matrix (read transposed, 4 next-states per thread, coalesced); the G previous rows
//                           double-buffered in LDS
//   stream_first_step_kernel  backpointers of ALL S states at the newest frame, one wave per state, many workgroups per
//                           stream (the only step of the walk that costs a full frame of cells)
//   stream_walk_kernel      one workgroup per stream: survivor-set walk from the newest frame back to the first pending one,
//                           stopping at the first frame whose set is a single state (the newest decided frame), then the
//                           backtrace from that state down to the first pending frame
// A flush is stream_walk_kernel with the final state (first NaN, otherwise first maximum) in place of the walk.
// A push with a maximum lag (torbi_hip_stream_push_lag) runs stream_walk_kernel<false, true>: where the walk leaves more than
// max_lag frames pending, the oldest of them are returned along the backtrace from the final state of the newest row.
//
// NaN and +/-inf need no second pass here.  The reference's scan (nonfinite.hpp::faithful_item) starts its running maximum at
// prev-state 0 and replaces it on a strict '>': a NaN candidate at prev-state 0 wins outright (value NaN, backpointer 0) and a
// NaN anywhere else never wins.  Candidates are sums, hence quiet NaNs, and v_max_f32 returns the other operand of a quiet
// NaN, so the reference's value is  isnan(c0) ? NaN : fmax over all candidates  and its backpointer is  isnan(c0) ? 0 : the
// first index of the largest non-NaN candidate.  Both are order-independent, so the parallel forms below are exact on any
// input (the sign of a zero maximum may differ; no comparison or later sum can tell).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace stream {

constexpr int kThreads = 256;
constexpr int kSentinel = 0x7fffffff;
constexpr int kMaxLdsBytes = 64 * 1024;
constexpr int kMaxStates = 8000;          // 2 * S words of dynamic LDS per workgroup (forward with G = 1, walk) below 64 KB

// info[b] of a call: what the host knows about stream b before it
struct Info {
    int32_t pending;      // frames pushed and not yet returned
    int32_t base_slot;    // ring slot of the first pending frame
    int32_t frames;       // frames in this push (push) / 1 = flush this stream (flush)
    int32_t fresh;        // 1: no frame pushed since the start or the last flush (the first row is obs[0] + initial)
};

__device__ __forceinline__ int slot_of(int base_slot, int r, int cap) {       // r >= -1
    return (base_slot + r + cap) % cap;
}

// info[b] fits a ring of `cap` slots to which the call adds `frames` (0 .. max_frames) rows, `room` = min(cap, out_cap)
// pending rows at the most afterwards: every slot_of() of the stream stays inside its ring, no pending row is overwritten
// and the output row holds whatever the call may return.  A stream that fails it is left alone by every kernel of the call
// (ring, memo and output row untouched) and reported as counts[b] = -1.
__device__ __forceinline__ bool info_fits(const Info &in, int frames, int max_frames, int cap, int room) {
    return in.pending >= 0 && in.base_slot >= 0 && in.base_slot < cap && frames >= 0 && frames <= max_frames &&
           in.pending <= room - frames;
}

// frames a push appends to a stream: info's count, 0 for a stream whose info does not fit
__device__ __forceinline__ int push_frames(const Info &in, int Tc, int cap, int room) {
    return info_fits(in, in.frames, Tc, cap, room) ? in.frames : 0;
}

// G streams of a tile: forward over `frames` new rows each.  obs (B, Tc, S); tt = transition transposed ([prev][next]);
// every thread owns J consecutive next-states (J = 4: S % 4 == 0, one 16-byte load of the matrix per prev-state feeds
// 4 * G cells).  Dynamic LDS: 2 * G * S floats.
template <int G, int J>
__global__ __launch_bounds__(kThreads) void stream_forward_kernel(const float *__restrict__ obs, int Tc, const Info *__restrict__ info,
                                                                  const float *__restrict__ tt, const float *__restrict__ initial,
                                                                  float *__restrict__ ring, int32_t *__restrict__ memo, int cap,
                                                                  int room, int B, int S) {
    extern __shared__ float rows[];          // [2][G][S]
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * G;
    int tmax = 0;
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (b0 + g < B) tmax = max(tmax, push_frames(info[b0 + g], Tc, cap, room));
    if (tmax == 0) return;
    // the carried rows
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int b = b0 + g;
        const bool carry = b < B && push_frames(info[b], Tc, cap, room) > 0 && !info[b].fresh;
        const float *src = carry ? ring + ((size_t)b * cap + slot_of(info[b].base_slot, info[b].pending - 1, cap)) * S : nullptr;
        for (int i = tid; i < S; i += kThreads) rows[(size_t)g * S + i] = carry ? src[i] : 0.f;
    }
    __syncthreads();
    for (int t = 0; t < tmax; ++t) {
        const float *cur = rows + (size_t)(t & 1) * G * S;
        float *nxt = rows + (size_t)((t + 1) & 1) * G * S;
        for (int j0 = tid * J; j0 < S; j0 += kThreads * J) {
            float acc[G][J];
            bool nan0[G][J];
            float tr[J];
            if (J == 4) {
                const float4 v = *reinterpret_cast<const float4 *>(tt + j0);
                tr[0] = v.x; tr[1 % J] = v.y; tr[2 % J] = v.z; tr[3 % J] = v.w;
            } else {
                tr[0] = tt[j0];
            }
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int q = 0; q < J; ++q) {
                    const float c = cur[(size_t)g * S] + tr[q];
                    nan0[g][q] = c != c;
                    acc[g][q] = c;
                }
#pragma unroll 4
            for (int i = 1; i < S; ++i) {
                if (J == 4) {
                    const float4 v = *reinterpret_cast<const float4 *>(tt + (size_t)i * S + j0);
                    tr[0] = v.x; tr[1 % J] = v.y; tr[2 % J] = v.z; tr[3 % J] = v.w;
                } else {
                    tr[0] = tt[(size_t)i * S + j0];
                }
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float p = cur[(size_t)g * S + i];
#pragma unroll
                    for (int q = 0; q < J; ++q) acc[g][q] = __builtin_fmaxf(acc[g][q], p + tr[q]);
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int b = b0 + g;
                if (b >= B) continue;
                const Info in = info[b];
                if (t >= push_frames(in, Tc, cap, room)) continue;
                float *dst = ring + ((size_t)b * cap + slot_of(in.base_slot, in.pending + t, cap)) * S;
#pragma unroll
                for (int q = 0; q < J; ++q) {
                    const int j = j0 + q;
                    const float o = obs[((size_t)b * Tc + t) * S + j];
                    const float v = (in.fresh && t == 0) ? o + initial[j] : o + (nan0[g][q] ? __builtin_nanf("") : acc[g][q]);
                    nxt[(size_t)g * S + j] = v;
                    dst[j] = v;
                }
            }
        }
        if (tid < G) {
            const int b = b0 + tid;
            if (b < B && t < push_frames(info[b], Tc, cap, room))
                memo[(size_t)b * cap + slot_of(info[b].base_slot, info[b].pending + t, cap)] = 0;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void take_better(float &v, int &i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__device__ __forceinline__ int wave_min(int x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = min(x, __shfl_xor(x, off, 64));
    return x;
}

// backpointer of state j at a frame whose previous row is `prev`: the reference's result (see the top of the file);
// one wave, every lane gets it
__device__ __forceinline__ int wave_backpointer(const float *__restrict__ prev, const float *__restrict__ trow, int S, int lane) {
    const float c0 = prev[0] + trow[0];
    if (c0 != c0) return 0;
    float best = -INFINITY;
    int arg = kSentinel;
    for (int i = lane; i < S; i += 64) {
        const float c = prev[i] + trow[i];
        if (c == c && (arg == kSentinel || c > best)) { best = c; arg = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(arg, off, 64);
        take_better(best, arg, ov, oi);
    }
    return arg;
}

// bp[b][j] = backpointer of state j at the newest frame of stream b, for every j: one wave per state (lanes over the
// prev-states of its matrix row, coalesced), grid = (ceil(S / 4), B).
__global__ __launch_bounds__(kThreads) void stream_first_step_kernel(const Info *__restrict__ info, const float *__restrict__ trans,
                                                                     const float *__restrict__ ring, int32_t *__restrict__ bp,
                                                                     int cap, int room, int Tc, int S) {
    const int b = blockIdx.y;
    const Info in = info[b];
    const int frames = push_frames(in, Tc, cap, room);
    const int P = in.pending + frames;
    if (frames <= 0 || P < 2 || S < 2) return;
    const int j = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= S) return;
    const float *prev = ring + ((size_t)b * cap + slot_of(in.base_slot, P - 2, cap)) * S;
    const int p = wave_backpointer(prev, trans + (size_t)j * S, S, lane);
    if (lane == 0) bp[(size_t)b * S + j] = p;
}

// final state of a row: its first NaN, otherwise its first maximum (ATen's argmax, viterbi.cpp:218); one wave
__device__ __forceinline__ int wave_final_state(const float *__restrict__ row, int S, int lane) {
    int first_nan = kSentinel;
    float best = -INFINITY;
    int arg = kSentinel;
    for (int i = lane; i < S; i += 64) {
        const float v = row[i];
        if (v != v) first_nan = min(first_nan, i);
        else if (arg == kSentinel || v > best) { best = v; arg = i; }
    }
    first_nan = wave_min(first_nan);
    if (first_nan < S) return first_nan;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(arg, off, 64);
        take_better(best, arg, ov, oi);
    }
    return arg;
}

// One workgroup per stream.  FLUSH = false: frontier walk + backtrace of the newly decided frames; FLUSH = true: final state +
// backtrace of every pending frame.  out[b][0 .. count) = the stream's frames base .. base + count - 1; counts[b] = count
// (-1: the call's info does not fit the ring (info_fits; Tc = frames a push may add) or the output, nothing written).
// LAG = true (push only): at most max_lag >= 0 frames stay pending.  Where the walk ends -- by any of its exits -- with
// c < P - 1 - max_lag, frames c + 1 .. P - 1 - max_lag are FORCED: one wave takes the final state of the newest row, follows
// the backpointers down to frame P - 1 - max_lag without storing and goes on as the backtrace of the whole returned span
// (every survivor shares the path up to c, so the decided frames come out as they would have).  forced[b] = frames of
// counts[b] that were forced (0 where counts[b] <= 0); without LAG neither max_lag nor forced is looked at.
// Dynamic LDS: 2 * S int32.
template <bool FLUSH, bool LAG = false>
__global__ __launch_bounds__(kThreads) void stream_walk_kernel(const Info *__restrict__ info, const float *__restrict__ trans,
                                                               const float *__restrict__ ring, int32_t *__restrict__ memo,
                                                               const int32_t *__restrict__ bp, int cap, int32_t *__restrict__ out,
                                                               int out_cap, int32_t *__restrict__ counts, int Tc, int S,
                                                               int max_lag, int32_t *__restrict__ forced) {
    static_assert(!(FLUSH && LAG), "a flush returns every pending frame: there is nothing to bound");
    extern __shared__ int32_t lds_i[];
    int32_t *flag = lds_i, *list = lds_i + S;
    __shared__ int32_t count_s, stop_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Info in = info[b];
    const int add = FLUSH ? 0 : in.frames;                      // rows the forward of this push appended
    const float *r0 = ring + (size_t)b * cap * S;
    int32_t *mb = memo + (size_t)b * cap;
    auto row = [&](int r) { return r0 + (size_t)slot_of(in.base_slot, r, cap) * S; };
    if (LAG && tid == 0) forced[b] = 0;
    if (in.frames == 0) { if (tid == 0) counts[b] = 0; return; }          // nothing asked of this stream
    if (!info_fits(in, add, FLUSH ? 0 : Tc, cap, min(cap, out_cap))) {
        if (tid == 0) counts[b] = -1;
        return;
    }
    const int P = in.pending + add;                             // pending frames after the forward of this push
    int c = -1, m = 0;                                  // newest decided frame (relative to base) and its state
    if (FLUSH) {
        if (P >= 1) {
            c = P - 1;
            if (wave == 0) m = wave_final_state(row(P - 1), S, lane);
        }
    } else if (S == 1) {
        c = P - 1;
    } else if (P >= 2) {
        for (int i = tid; i < S; i += kThreads) flag[i] = 0;
        if (tid == 0) stop_s = 0;
        __syncthreads();
        // the set at frame P-2: the image of the newest frame's backpointers
        for (int j = tid; j < S; j += kThreads) flag[bp[(size_t)b * S + j]] = 1;
        for (int f = P - 2; ; --f) {                    // f: frame whose set is in `flag`
            if (tid == 0) count_s = 0;
            __syncthreads();
            for (int i = tid; i < S; i += kThreads)
                if (flag[i]) { list[atomicAdd(&count_s, 1)] = i; flag[i] = 0; }
            __syncthreads();
            const int k = count_s;
            if (k == 1) { c = f; m = list[0]; break; }
            // a set of the same size as the one an earlier walk found here is that set (this one is a subset of it), and
            // that walk found no single state at or below this frame
            const bool same = mb[slot_of(in.base_slot, f, cap)] == k;
            __syncthreads();
            if (tid == 0) mb[slot_of(in.base_slot, f, cap)] = k;
            if (same || f == 0) break;
            const float *prev = row(f - 1);
            for (int q = wave; q < k; q += kThreads / 64) {
                const int j = list[q];
                const int p = wave_backpointer(prev, trans + (size_t)j * S, S, lane);
                if (lane == 0) flag[p] = 1;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (LAG && c < P - 1 - max_lag) {                   // (uniform: c, P and max_lag are the same in every thread)
        const int target = P - 1 - max_lag;             // >= 0
        if (tid == 0) forced[b] = target - c;
        c = target;
        if (wave == 0) {
            m = wave_final_state(row(P - 1), S, lane);
            for (int f = P - 1; f > target; --f) m = wave_backpointer(row(f - 1), trans + (size_t)m * S, S, lane);
        }
    }
    if (tid == 0) counts[b] = c + 1;
    if (wave != 0 || c < 0) return;
    // backtrace: frames c, c-1, ..., 0 of the pending span
    m = __shfl(m, 0, 64);
    int32_t *o = out + (size_t)b * out_cap;
    if (lane == 0) o[c] = m;
    for (int f = c; f >= 1; --f) {
        m = wave_backpointer(row(f - 1), trans + (size_t)m * S, S, lane);
        if (lane == 0) o[f - 1] = m;
    }
}

}  // namespace stream
