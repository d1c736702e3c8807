// stream_band.hpp -- the band route of streaming decode (torbi_hip_stream_band_*, torbi_amd/stream.py, STREAM.md "Band route"):
// stream.hpp's decoder, bit for bit, for a matrix that holds ONE value outside a band, at the cost of the band.
//
// The rule is stream.hpp's: candidates c_i = fl(prev[i] + A[j][i]),  value = isnan(c_0) ? NaN : max of the non-NaN candidates,
// backpointer = isnan(c_0) ? 0 : first index of the largest non-NaN candidate.  With A[j][i] = background for i outside
// [j - reach_left, j + reach_right], every out-of-band candidate of every state j is d_i = fl(prev[i] + background), so
//     pre[i] = the best non-NaN (d, index) over 0 .. i          suf[i] = the best over i .. S - 1
// ("best" = take_better: larger value, then lower index; "none" = (-inf, kSentinel) for a range without a non-NaN entry,
// which every real entry beats and which beats nothing) are two scans per frame and stream, and state j combines
// pre[j - reach_left - 1], its W = reach_left + reach_right + 1 in-band candidates in ascending i and suf[j + reach_right + 1],
// each on a strict '>'.  take_better is a lexicographic maximum, hence associative and commutative: the result is the first
// index of the largest non-NaN candidate whatever the grouping.  A strict '>' from "none" never takes a -inf candidate, so a
// state that ends without an index (all its non-NaN candidates are -inf) takes the first non-NaN one: the prefix's index,
// else the first in-band one, else the suffix's.  The NaN test of c_0 uses the in-band entry when j <= reach_left, d_0
// otherwise.  One code path for a finite background and for -inf (+inf beside -inf gives a NaN candidate, which is skipped).
//
// The arg-max comes with the maximum, so the forward STORES each frame's backpointers; the frontier walk, the forced-lag
// chain and the backtrace only follow stored pointers.  State (torbi_hip_stream_state_bytes, the dense route's size):
//     ring    [B][cap][S] int32  backpointers of the pending frames; frame `base + r` lives in slot (base_slot + r) % cap
//                                (the row of relative frame 0 is never read)
//     memo    [B][cap]    int32  as stream.hpp
//     carried [B][S]      fp32   the newest posterior row
// A push is two launches (stream_band_forward_kernel, stream_band_walk_kernel<false, LAG>), a flush one
// (stream_band_walk_kernel<true>).  The diagonals diag[k][j] = A[j][j - reach_left + k], [W][S], are extracted once per
// matrix by banddiag::prepare_kernel (band_diagonals.hpp), which also checks the caller's promise about the entries outside
// the band.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "band_diagonals.hpp"
#include "stream.hpp"

namespace stream_band {

using stream::Info;
using stream::info_fits;
using stream::kSentinel;
using stream::kThreads;
using stream::push_frames;
using stream::slot_of;
using stream::take_better;
using stream::wave_final_state;

constexpr int kMaxGroup = 4;                    // streams per workgroup: instances <1>, <2>, <4>
constexpr int kMaxLdsBytes = banddiag::kMaxLdsBytes;
constexpr int kForwardThreads = 1024;           // of the forward kernel: sixteen waves hide the L2 latency of the diagonals

// floats of one stream's row with its NaN halos
__host__ __device__ inline size_t row_words(int S, int reach_left, int reach_right) { return (size_t)S + reach_left + reach_right; }

// dynamic LDS of stream_band_forward_kernel<G>: rows [2][G][reach_left + S + reach_right] fp32, then per stream the scans
// pre value [S] fp32, pre index [S] int32, suf value [S], suf index [S]
__host__ __device__ inline size_t lds_bytes(int G, int S, int reach_left, int reach_right) {
    return ((size_t)2 * G * row_words(S, reach_left, reach_right) + (size_t)4 * G * S) * 4;
}

// inclusive scan of take_better over the lanes of a wave, towards higher lanes (UP) or lower ones
template <bool UP>
__device__ __forceinline__ void wave_scan(float &v, int &i, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float ov = UP ? __shfl_up(v, off, 64) : __shfl_down(v, off, 64);
        const int oi = UP ? __shfl_up(i, off, 64) : __shfl_down(i, off, 64);
        if (UP ? lane >= off : lane + off < 64) take_better(v, i, ov, oi);
    }
}

// G streams of a tile: the band recurrence over `frames` new rows each, all frames of the push in one launch.
// obs (B, Tc, S); diag [W][S] (banddiag::prepare_kernel).  A thread owns next-states j = tid + 1024 * m; the G streams share
// every load of a diagonal entry.  Per frame: both scans of the G previous rows (each thread a run of consecutive states,
// the runs joined by a wave scan and the sixteen wave totals), then the band.
template <int G>
__global__ __launch_bounds__(kForwardThreads) void stream_band_forward_kernel(const float *__restrict__ obs, int Tc, const Info *__restrict__ info,
                                                                       const float *__restrict__ diag, const float *__restrict__ initial,
                                                                       float background, int reach_left, int reach_right,
                                                                       int32_t *__restrict__ ring, int32_t *__restrict__ memo,
                                                                       float *__restrict__ carried, int cap, int room, int B, int S) {
    extern __shared__ float lds_f[];
    __shared__ float tot_v[2][G][kForwardThreads / 64];
    __shared__ int tot_i[2][G][kForwardThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * G;
    const int W = reach_left + reach_right + 1;
    const size_t RW = row_words(S, reach_left, reach_right);
    float *rows = lds_f;                                        // [2][G][RW]
    float *scan = lds_f + (size_t)2 * G * RW;                   // [G][4][S]
    int frames_of[G];
    int tmax = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        frames_of[g] = b0 + g < B ? push_frames(info[b0 + g], Tc, cap, room) : 0;
        tmax = max(tmax, frames_of[g]);
    }
    if (tmax == 0) return;
    // NaN halos of both buffers, and the carried rows
    for (int x = tid; x < 2 * G * (reach_left + reach_right); x += kForwardThreads) {
        const int r = x / (reach_left + reach_right), h = x % (reach_left + reach_right);
        rows[(size_t)r * RW + (h < reach_left ? h : S + h)] = __builtin_nanf("");
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const bool carry = frames_of[g] > 0 && !info[b0 + g].fresh;
        const float *src = carried + (size_t)(b0 + g) * S;
        for (int i = tid; i < S; i += kForwardThreads) rows[(size_t)g * RW + reach_left + i] = carry ? src[i] : 0.f;
    }
    __syncthreads();
    const int chunk = (S + kForwardThreads - 1) / kForwardThreads;
    const int lo = min(tid * chunk, S), hi = min(lo + chunk, S);
    for (int t = 0; t < tmax; ++t) {
        const float *cur = rows + (size_t)(t & 1) * G * RW + reach_left;          // cur[g * RW + i], i in -reach_left .. S + reach_right - 1
        float *nxt = rows + (size_t)((t + 1) & 1) * G * RW + reach_left;
        // ---- the scans of d_i = prev[i] + background
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float *p = cur + (size_t)g * RW;
            float *pv = scan + (size_t)g * 4 * S, *sv = pv + 2 * S;
            int *pi = reinterpret_cast<int *>(pv + S), *si = reinterpret_cast<int *>(sv + S);
            float v = -INFINITY;
            int a = kSentinel;
            for (int i = lo; i < hi; ++i) {
                const float d = p[i] + background;
                if (d == d) take_better(v, a, d, i);
                pv[i] = v;
                pi[i] = a;
            }
            float ev = v;
            int ea = a;
            wave_scan<true>(ev, ea, lane);
            if (lane == 63) { tot_v[0][g][wave] = ev; tot_i[0][g][wave] = ea; }
            // this thread's offset within its wave: the lanes below
            float xv = __shfl_up(ev, 1, 64);
            int xa = __shfl_up(ea, 1, 64);
            if (lane == 0) { xv = -INFINITY; xa = kSentinel; }
            v = -INFINITY;
            a = kSentinel;
            for (int i = hi - 1; i >= lo; --i) {
                const float d = p[i] + background;
                if (d == d) take_better(v, a, d, i);
                sv[i] = v;
                si[i] = a;
            }
            float fv = v;
            int fa = a;
            wave_scan<false>(fv, fa, lane);
            if (lane == 0) { tot_v[1][g][wave] = fv; tot_i[1][g][wave] = fa; }
            float yv = __shfl_down(fv, 1, 64);
            int ya = __shfl_down(fa, 1, 64);
            if (lane == 63) { yv = -INFINITY; ya = kSentinel; }
            __syncthreads();
            for (int w = 0; w < wave; ++w) take_better(xv, xa, tot_v[0][g][w], tot_i[0][g][w]);
            for (int w = wave + 1; w < kForwardThreads / 64; ++w) take_better(yv, ya, tot_v[1][g][w], tot_i[1][g][w]);
            for (int i = lo; i < hi; ++i) {
                float qv = pv[i];
                int qa = pi[i];
                take_better(qv, qa, xv, xa);
                pv[i] = qv;
                pi[i] = qa;
                qv = sv[i];
                qa = si[i];
                take_better(qv, qa, yv, ya);
                sv[i] = qv;
                si[i] = qa;
            }
        }
        __syncthreads();
        // ---- the band
        for (int j = tid; j < S; j += kForwardThreads) {
            float best[G];
            int arg[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float *pv = scan + (size_t)g * 4 * S;
                const int e = j - reach_left - 1;
                best[g] = e >= 0 ? pv[e] : -INFINITY;
                arg[g] = e >= 0 ? reinterpret_cast<const int *>(pv + S)[e] : kSentinel;
            }
            const float *dj = diag + j;
            const float *pj = cur + j - reach_left;
            constexpr int U = G == 4 ? 4 : 8;            // diagonal loads in flight per thread (registers: 128 at 1024 threads)
            int k = 0;
            for (; k + U <= W; k += U) {
                float dv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) dv[u] = dj[(size_t)(k + u) * S];
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const float c = pj[(size_t)g * RW + k + u] + dv[u];
                        if (c > best[g]) { best[g] = c; arg[g] = j - reach_left + k + u; }
                    }
            }
            for (; k < W; ++k) {
                const float dv = dj[(size_t)k * S];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float c = pj[(size_t)g * RW + k] + dv;
                    if (c > best[g]) { best[g] = c; arg[g] = j - reach_left + k; }
                }
            }
            const float first = j <= reach_left ? dj[(size_t)(reach_left - j) * S] : background;       // A[j][0]
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float *sv = scan + (size_t)g * 4 * S + 2 * S;
                const int e = j + reach_right + 1;
                const float ov = e < S ? sv[e] : -INFINITY;
                const int oi = e < S ? reinterpret_cast<const int *>(sv + S)[e] : kSentinel;
                if (ov > best[g]) { best[g] = ov; arg[g] = oi; }
                if (arg[g] == kSentinel) {
                    // every non-NaN candidate is -inf (and the prefix has none): the first of them
                    for (int q = 0; q < W && arg[g] == kSentinel; ++q) {
                        const float c = pj[(size_t)g * RW + q] + dj[(size_t)q * S];
                        if (c == c) arg[g] = j - reach_left + q;
                    }
                    if (arg[g] == kSentinel) arg[g] = oi;
                }
                const float c0 = cur[(size_t)g * RW] + first;
                const bool nan0 = c0 != c0;
                const int b = b0 + g;
                if (t < frames_of[g]) {
                    const Info in = info[b];
                    const bool start = in.fresh && t == 0;
                    const float o = obs[((size_t)b * Tc + t) * S + j];
                    const float v = start ? o + initial[j] : o + (nan0 ? __builtin_nanf("") : best[g]);
                    nxt[(size_t)g * RW + j] = v;
                    if (!start)
                        ring[((size_t)b * cap + slot_of(in.base_slot, in.pending + t, cap)) * S + j] =
                            (nan0 || arg[g] == kSentinel) ? 0 : arg[g];
                    if (t == frames_of[g] - 1) carried[(size_t)b * S + j] = v;
                }
            }
        }
        if (tid < G && b0 + tid < B && t < push_frames(info[b0 + tid], Tc, cap, room)) {
            const Info in = info[b0 + tid];
            memo[(size_t)(b0 + tid) * cap + slot_of(in.base_slot, in.pending + t, cap)] = 0;
        }
        __syncthreads();
    }
}

// stream.hpp's stream_walk_kernel on stored pointers: one workgroup per stream, the same exits, counts and forced counts;
// every backpointer is a read of ring[slot of its frame][state].  The set at frame P - 2 is the image of the stored row of
// frame P - 1; flush and the forced arm take the final state of the carried row.  Dynamic LDS: 2 * S int32.
template <bool FLUSH, bool LAG = false>
__global__ __launch_bounds__(kThreads) void stream_band_walk_kernel(const Info *__restrict__ info, const int32_t *__restrict__ ring,
                                                                    int32_t *__restrict__ memo, const float *__restrict__ carried,
                                                                    int cap, int32_t *__restrict__ out, int out_cap,
                                                                    int32_t *__restrict__ counts, int Tc, int S, int max_lag,
                                                                    int32_t *__restrict__ forced) {
    static_assert(!(FLUSH && LAG), "a flush returns every pending frame: there is nothing to bound");
    extern __shared__ int32_t lds_w[];
    int32_t *flag = lds_w, *list = lds_w + S;
    __shared__ int32_t count_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Info in = info[b];
    const int add = FLUSH ? 0 : in.frames;
    const int32_t *r0 = ring + (size_t)b * cap * S;
    int32_t *mb = memo + (size_t)b * cap;
    const float *newest = carried + (size_t)b * S;
    // the pointer of state j at frame r into frame r - 1 (kept inside the row whatever the caller's state holds)
    auto ptr = [&](int r, int j) { return min(max(r0[(size_t)slot_of(in.base_slot, r, cap) * S + j], 0), S - 1); };
    if (LAG && tid == 0) forced[b] = 0;
    if (in.frames == 0) { if (tid == 0) counts[b] = 0; return; }
    if (!info_fits(in, add, FLUSH ? 0 : Tc, cap, min(cap, out_cap))) {
        if (tid == 0) counts[b] = -1;
        return;
    }
    const int P = in.pending + add;
    int c = -1, m = 0;
    if (FLUSH) {
        if (P >= 1) {
            c = P - 1;
            if (wave == 0) m = wave_final_state(newest, S, lane);
        }
    } else if (S == 1) {
        c = P - 1;
    } else if (P >= 2) {
        for (int i = tid; i < S; i += kThreads) flag[i] = 0;
        __syncthreads();
        for (int j = tid; j < S; j += kThreads) flag[ptr(P - 1, j)] = 1;
        for (int f = P - 2; ; --f) {                    // f: frame whose set is in `flag`
            if (tid == 0) count_s = 0;
            __syncthreads();
            for (int i = tid; i < S; i += kThreads)
                if (flag[i]) { list[atomicAdd(&count_s, 1)] = i; flag[i] = 0; }
            __syncthreads();
            const int k = count_s;
            if (k == 1) { c = f; m = list[0]; break; }
            const bool same = mb[slot_of(in.base_slot, f, cap)] == k;
            __syncthreads();
            if (tid == 0) mb[slot_of(in.base_slot, f, cap)] = k;
            if (same || f == 0) break;
            for (int q = tid; q < k; q += kThreads) flag[ptr(f, list[q])] = 1;
            __syncthreads();
        }
    }
    __syncthreads();
    if (LAG && c < P - 1 - max_lag) {
        const int target = P - 1 - max_lag;             // >= 0
        if (tid == 0) forced[b] = target - c;
        c = target;
        if (wave == 0) {
            m = wave_final_state(newest, S, lane);
            for (int f = P - 1; f > target; --f) m = ptr(f, m);
        }
    }
    if (tid == 0) counts[b] = c + 1;
    if (wave != 0 || c < 0) return;
    m = __shfl(m, 0, 64);
    int32_t *o = out + (size_t)b * out_cap;
    if (lane == 0) {
        o[c] = m;
        for (int f = c; f >= 1; --f) {
            m = ptr(f, m);
            o[f - 1] = m;
        }
    }
}

}  // namespace stream_band
