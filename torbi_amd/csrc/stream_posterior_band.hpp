// stream_posterior_band.hpp -- the band route of streaming posteriors: stream_posterior.hpp's recurrence, state and Info rule
// for a transition matrix that holds ONE value outside a band (torbi_hip_stream_smooth_band_*, torbi_amd/stream_posterior.py,
// STREAM.md "Streaming posteriors: band route").  The streaming twin of fb_band_kernel (forward_backward_band.hpp): the same
// split of the two matrix products, the same diagonals, the same ownership of states and the same reductions.
//
// The caller states a band j - reach_left <= i <= j + reach_right of A [next j][prev i] and a `background`.  With
// ebg = exp(background) (0 for -inf):
//     forward   (E a)[j]   = sum_k Df[k][j] * a[j - reach_left + k]  +  ebg * c_{t-1}       (c_{t-1} is already in the ring)
//     backward  (E^T w)[i] = sum_k Db[k][i] * w[i + reach_left - k]  +  ebg * sum_j w[j]     (the sum only where ebg != 0)
// No product is skipped: an in-band NaN or +inf reaches every stream that takes a second frame.
//
// The diagonals ([2][W][Sd] fp32, Df then Db, W = reach_left + reach_right + 1 with the reaches clamped to S - 1, Sd = S up to
// 64) are fbb::fb_band_prepare_kernel's, the promise is checked by fbb::fb_band_verify_kernel; spb_verdict_kernel turns
// their flag into the verdict the caller reads.  The state is stream_posterior.hpp's, bit for bit.
//
// A push is two launches, a flush the second alone; a workgroup of 1024 threads owns G whole streams, thread `tid` owns states
// tid, tid + 1024, ... of each of them:
//   spb_forward_kernel<G>   first m_t of every new frame (one wave per row, straight into the ring), then the scaled
//                           recurrence over every frame of the push: the rows a_{t-1} / a_t in LDS with zero halos, the
//                           diagonals from L2 (every load shared by the G streams), one barrier per frame
//   spb_backward_kernel<G>  one sweep from frame n' - 1 down to base; the w rows double-buffered in LDS with halos; only the
//                           rows that leave are written.  A stream that returns nothing takes no step.
// In both the frame's own rows (the observation; e_t and a_t) are requested before the band sum and used after it.
//
// A stream's bits depend on its own data and (t, n') only -- not on G, the ring slot, the cut into pushes or its neighbours:
// a band sum is one fmaf chain over k = 0 .. W - 1; c_t and sum_j w[j] are a thread's states in order, a 64-lane butterfly per
// wave and a 16-lane butterfly over the 16 wave sums; the row maximum is order-free; L is one fp64 add per frame.
// Vector stores only, no float atomics, nothing waits across workgroups, no host synchronisation.
#pragma once

#include "stream_posterior.hpp"
#include "forward_backward_band.hpp"

namespace spb {

using stream::Info;
using stream::slot_of;
namespace sp = stream_posterior;

constexpr int kThreads = fbb::kThreads, kWaves = fbb::kWaves;
constexpr int kMaxStates = fbb::kMaxStates;
constexpr int kMaxWindow = fbb::kMaxWindow;
constexpr int kMaxGroup = 8;                 // streams per workgroup: the largest tile whose kernels need no scratch
constexpr int kMaxLdsBytes = 64 * 1024;

// LDS of a tile of G streams: the rows [2][G][S + 2 halo] and the wave sums [2][G][16], fp32
inline size_t lds_bytes(int G, int S, int halo) { return (size_t)2 * G * (fbb::row_stride(S, halo) + kWaves) * sizeof(float); }

// 1 where the promise holds (flag: what fb_band_prepare_kernel reset and fb_band_verify_kernel raised)
__global__ void spb_verdict_kernel(int32_t *flag) { *flag = *flag == 0 ? 1 : 0; }

// ---- forward: G streams of a tile, `frames` new rows each.  obs (B, Tc, S).  Dynamic LDS: lds_bytes(G, S, halo) ----
template <int G>
__global__ __launch_bounds__(kThreads) void spb_forward_kernel(const float *__restrict__ obs, int Tc, const Info *__restrict__ info,
                                                               const float *__restrict__ Df, const float *__restrict__ initial,
                                                               int32_t *__restrict__ Lw, float *__restrict__ ring_a,
                                                               float *__restrict__ ring_e, float *__restrict__ ring_c,
                                                               float *__restrict__ ring_m, float ebg, int reach_left, int halo,
                                                               int W, int Sd, int cap, int out_cap, int lag, int B, int S) {
    extern __shared__ float lds[];
    constexpr int kUnroll = fbb::band_unroll(G);
    const int stride = fbb::row_stride(S, halo);
    float *const rows = lds;                                 // [2][G][stride]
    float *const part = lds + (size_t)2 * G * stride;        // [2][G][16] wave sums of a row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * G;
    int fr[G], tmax = 0;
    Info in[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        in[g] = b0 + g < B ? info[b0 + g] : Info{0, 0, 0, 0};
        fr[g] = b0 + g < B ? sp::new_frames(in[g], Tc, cap, out_cap, lag) : 0;
        tmax = max(tmax, fr[g]);
    }
    if (tmax == 0) return;
    for (int e = tid; e < 2 * G * stride; e += kThreads) rows[e] = 0.f;      // (the halos stay zero all launch long)
    __syncthreads();
    // the carried rows (frame -1 lives where frame 1 will) and their sums
    float cprev[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const bool carry = fr[g] > 0 && !in[g].fresh;
        const size_t at = (size_t)(b0 + g) * cap + (carry ? slot_of(in[g].base_slot, in[g].pending - 1, cap) : 0);
        if (carry)
            for (int i = tid; i < S; i += kThreads) rows[(size_t)(G + g) * stride + halo + i] = ring_a[at * S + i];
        cprev[g] = carry ? ring_c[at] : 1.f;
    }
    double L = 0.;                           // thread g carries the running sum of stream g
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (tid == g && fr[g] > 0 && !in[g].fresh) L = sp::load_sum(Lw + 2 * (size_t)(b0 + g));
    // m_t of every new frame, one wave per row: the NaN-propagating maximum (initial added on a stream's first frame), -inf
    // read as 0
#pragma unroll
    for (int g = 0; g < G; ++g) {
        for (int t = wave; t < fr[g]; t += kWaves) {
            const float *o = obs + ((size_t)(b0 + g) * Tc + t) * S;
            const bool first = in[g].fresh && t == 0;
            float best = -INFINITY;
            int nan = 0;
#pragma unroll 8
            for (int i = lane; i < S; i += 64) {
                const float x = first ? initial[i] + o[i] : o[i];
                nan |= x != x;
                best = __builtin_fmaxf(best, x);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                best = __builtin_fmaxf(best, __shfl_xor(best, off, 64));
                nan |= __shfl_xor(nan, off, 64);
            }
            if (lane == 0)
                ring_m[(size_t)(b0 + g) * cap + slot_of(in[g].base_slot, in[g].pending + t, cap)] =
                    nan ? __builtin_nanf("") : (best == -INFINITY ? 0.f : best);
        }
    }
    __syncthreads();                                             // (the rows, and m_t written by one lane is read by all below)
    for (int t = 0; t <= tmax; ++t) {
        if (t > 0) {
            // c_{t-1} from the wave sums, the same bits in every lane; thread g stores it and adds the frame's term to L
            const float *p = part + (size_t)((t - 1) & 1) * G * kWaves;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t - 1 >= fr[g]) continue;
                const float c = fbb::sum16(p[g * kWaves + (lane & 15)]);
                cprev[g] = c;
                if (tid == g) {
                    const size_t at = (size_t)(b0 + g) * cap + slot_of(in[g].base_slot, in[g].pending + t - 1, cap);
                    ring_c[at] = c;
                    L += log((double)c) + (double)ring_m[at];
                }
            }
        }
        if (t == tmax) break;
        float *cur = rows + (size_t)(t & 1) * G * stride;
        const float *prev = rows + (size_t)((t & 1) ^ 1) * G * stride;
        float mt[G], acc[G];
        size_t at[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            acc[g] = 0.f;
            at[g] = (size_t)(b0 + g) * cap + (t < fr[g] ? slot_of(in[g].base_slot, in[g].pending + t, cap) : 0);
            mt[g] = t < fr[g] ? ring_m[at[g]] : 0.f;
        }
        for (int j = tid; j < S; j += kThreads) {
            float s[G], ot[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                s[g] = 0.f;
                ot[g] = t < fr[g] ? obs[((size_t)(b0 + g) * Tc + t) * S + j] : 0.f;        // (in flight during the band sum)
            }
            const float *d = Df + j;
            const float *x = prev + halo - reach_left + j;
#pragma unroll kUnroll
            for (int k = 0; k < W; ++k) {
                const float dk = d[(size_t)k * Sd];
#pragma unroll
                for (int g = 0; g < G; ++g) s[g] = fmaf(dk, x[g * stride + k], s[g]);
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t >= fr[g]) continue;
                const bool first = in[g].fresh && t == 0;
                const float e = expf((first ? initial[j] + ot[g] : ot[g]) - mt[g]);
                float v = e;
                if (!first) {
                    const float c = cprev[g];
                    const float u = e * (ebg != 0.f ? fmaf(ebg, c, s[g]) : s[g]);
                    v = c == 0.f ? u * 0.f : u / c;                  // (after a zero-probability frame: 0, or NaN from NaN)
                }
                cur[g * stride + halo + j] = v;
                ring_a[at[g] * S + j] = v;
                ring_e[at[g] * S + j] = e;
                acc[g] += v;
            }
        }
        float *p = part + (size_t)(t & 1) * G * kWaves;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float a = fbb::wave_sum(acc[g]);
            if (lane == 0) p[g * kWaves + wave] = a;
        }
        __syncthreads();
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (tid == g && fr[g] > 0) sp::store_sum(Lw + 2 * (size_t)(b0 + g), L);
}

// ---- backward: G streams of a tile, one sweep from the newest frame down to the first pending one.  Tc >= 0: the second
// launch of a push (the forward has appended info.frames rows); Tc < 0: a flush (info.frames = 1 flags the stream).  out
// [B][out_cap][S]: rows 0 .. count - 1 are the stream's frames base .. base + count - 1; counts (may be null) [B] = count, -1
// where the info does not fit.  NaN rows where the stream's running sum is not finite.  Dynamic LDS: lds_bytes(G, S, halo) ----
template <int G>
__global__ __launch_bounds__(kThreads) void spb_backward_kernel(const Info *__restrict__ info, int Tc, const float *__restrict__ Db,
                                                                const int32_t *__restrict__ Lw, const float *__restrict__ ring_a,
                                                                const float *__restrict__ ring_e, const float *__restrict__ ring_c,
                                                                float ebg, int reach_left, int halo, int W, int Sd, int cap,
                                                                float *__restrict__ out, int out_cap, int32_t *__restrict__ counts,
                                                                int lag, int B, int S) {
    extern __shared__ float lds[];
    constexpr int kUnroll = fbb::band_unroll(G);
    const int stride = fbb::row_stride(S, halo);
    float *const rows = lds;                                 // [2][G][stride]: w of the step before, w of this step
    float *const part = lds + (size_t)2 * G * stride;        // [2][G][16] wave sums of a w row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * G;
    const bool flush = Tc < 0;
    int P[G], count[G], kmax = 0;
    bool bad[G];
    Info in[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const bool here = b0 + g < B;
        in[g] = here ? info[b0 + g] : Info{0, 0, 0, 0};
        const bool ok = here && sp::call_fits(in[g], Tc, cap, out_cap, lag);
        const bool asked = ok && in[g].frames != 0;
        P[g] = asked ? in[g].pending + (flush ? 0 : in[g].frames) : 0;
        count[g] = asked ? (flush ? in[g].pending : sp::leaving(in[g], in[g].frames, lag)) : 0;
        if (count[g] == 0) P[g] = 0;                                 // nothing leaves: no step
        if (here && counts && tid == 0) counts[b0 + g] = ok ? count[g] : -1;
        kmax = max(kmax, P[g]);
        bad[g] = false;
        if (P[g] > 0) {
            const double L = sp::load_sum(Lw + 2 * (size_t)(b0 + g));
            bad[g] = !(L == L) || L == (double)INFINITY || L == -(double)INFINITY;
        }
    }
    if (kmax == 0) return;
    for (int e = tid; e < 2 * G * stride; e += kThreads) rows[e] = 0.f;      // (the halos stay zero all launch long)
    __syncthreads();
    for (int k = 0; k < kmax; ++k) {
        const float *prev = rows + (size_t)(k & 1) * G * stride;
        float *cur = rows + (size_t)((k + 1) & 1) * G * stride;
        float sw[G], acc[G], ct[G];
        size_t row[G];
        int r[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            sw[g] = acc[g] = 0.f;
            r[g] = P[g] - 1 - k;                                     // the frame of this step, relative to base
            row[g] = (size_t)(b0 + g) * cap + (k < P[g] ? slot_of(in[g].base_slot, r[g], cap) : 0);
            ct[g] = k < P[g] ? ring_c[row[g]] : 1.f;
        }
        if (ebg != 0.f && k > 0) {
            const float *p = part + (size_t)(k & 1) * G * kWaves;
#pragma unroll
            for (int g = 0; g < G; ++g) sw[g] = fbb::sum16(p[g * kWaves + (lane & 15)]);
        }
        for (int i = tid; i < S; i += kThreads) {
            float s[G], et[G], at[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                s[g] = 0.f;
                et[g] = k < P[g] ? ring_e[row[g] * S + i] : 0.f;                       // (in flight during the band sum)
                at[g] = k < P[g] && r[g] < count[g] ? ring_a[row[g] * S + i] : 0.f;
            }
            if (k > 0) {
                const float *d = Db + i;
                const float *x = prev + halo + reach_left + i;
#pragma unroll kUnroll
                for (int q = 0; q < W; ++q) {
                    const float dq = d[(size_t)q * Sd];
#pragma unroll
                    for (int g = 0; g < G; ++g) s[g] = fmaf(dq, x[g * stride - q], s[g]);
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (k >= P[g]) continue;
                const float beta = k == 0 ? 1.f : (ebg != 0.f ? fmaf(ebg, sw[g], s[g]) : s[g]);
                const float w = (et[g] * beta) / ct[g];
                cur[g * stride + halo + i] = w;
                acc[g] += w;
                if (r[g] < count[g])
                    out[((size_t)(b0 + g) * out_cap + r[g]) * S + i] = bad[g] ? __builtin_nanf("") : (at[g] * beta) / ct[g];
            }
        }
        if (ebg != 0.f) {
            float *p = part + (size_t)((k + 1) & 1) * G * kWaves;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float a = fbb::wave_sum(acc[g]);
                if (lane == 0) p[g * kWaves + wave] = a;
            }
        }
        __syncthreads();
    }
}

}  // namespace spb
