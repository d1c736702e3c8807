// forward_backward_band.hpp -- state posteriors and log-likelihood for a transition matrix that holds ONE value outside a
// band (torbi_hip_forward_backward_band, torbi_amd/posterior.py forward_backward_banded, POSTERIOR.md "Band route").
//
// The model, the contract and the scaled recurrence are forward_backward.hpp's.  The caller states a band
// j - reach_left <= i <= j + reach_right of A [next j][prev i] and a `background`: every entry outside the band equals
// `background` bit for bit.  With ebg = exp(background) (0 for -inf) each product splits into the band and one constant:
//     forward   (E a)[j]   = sum_{i in band(j)}  (E[j,i] - ebg) a[i]  +  ebg * sum_i a[i]        (sum_i a[i] = c_{t-1})
//     backward  (E^T w)[i] = sum_{j: i in band(j)} (E[j,i] - ebg) w[j]  +  ebg * sum_j w[j]
// so a step costs W = reach_left + reach_right + 1 multiplies per state where the dense route spends S.
//
// Workspace (torbi_hip_forward_backward_band_workspace_bytes), every piece 256-B aligned, Sd = S up to 64:
//     Df   [W][Sd] fp32   Df[k][j] = E[j][j - reach_left + k] - ebg     (forward: diagonal k along the next state)
//     Db   [W][Sd] fp32   Db[k][i] = E[i + reach_left - k][i] - ebg     (backward: the same diagonal along the prev state)
//                         positions clipped at the matrix edges are 0
//     m    [B][T]  fp32   row maxima (fb_rowmax_kernel)
//     c    [B][T]  fp32   row sums c_t
//     flag int32          1 when an entry outside the stated band differs from `background`
//
// fb_band_kernel<G>: ONE launch runs all T frames of both passes.  A workgroup of 1024 threads owns G whole items, so
// nothing waits across workgroups; thread `tid` owns states tid, tid + 1024, ... of every item of the tile in both passes.
// The rows a_{t-1} / a_t (then w_{t+1} / w_t) of the tile live in LDS with a zero halo of max(reach) on both sides, the
// diagonals stream from L2 and every load of one is shared by the G items.  One barrier per frame and pass.
//
// Reductions, per item and in a fixed order that does not depend on G: the states of a wave by a 64-lane butterfly, the
// 16 wave sums by a 16-lane butterfly (every lane of every wave computes the same bits); L as in fb_loglik_kernel over
// t = tid, tid + 1024, ... in fp64, a butterfly per wave, the 16 wave sums in order.  No float atomics, vector stores only.
#pragma once

#include "band_diagonals.hpp"
#include "forward_backward.hpp"

namespace fbb {

constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr int kMaxStates = 4096;
constexpr int kMaxWindow = 64;               // in-band entries of one matrix row: min(W, S) <= 64
constexpr int kMaxGroup = 8;                 // items per workgroup (16 would not fit 128 VGPRs without scratch)
constexpr int kMaxLdsBytes = 64 * 1024;

__host__ __device__ inline int clamp_reach(int reach, int S) { return reach < 0 ? 0 : (reach > S - 1 ? S - 1 : reach); }

// what the band is to the kernels, one-shot and streaming (stream_posterior_band.hpp): the reaches clamped to S - 1, the
// diagonals [W][Sd], the zero halo of the LDS rows
struct Band { int reach_left, reach_right, W, Sd, halo; };
inline Band band_of(int S, int reach_left, int reach_right) {
    Band b;
    b.reach_left = clamp_reach(reach_left, S);
    b.reach_right = clamp_reach(reach_right, S);
    b.W = b.reach_left + b.reach_right + 1;
    b.Sd = (int)align_up((size_t)S, 64);
    b.halo = b.reach_left > b.reach_right ? b.reach_left : b.reach_right;
    return b;
}

struct Layout : Band { float *Df, *Db, *m, *c; int32_t *flag; size_t total; };

// `base`: the caller's workspace aligned up to 256 bytes, or null for the byte count alone
inline Layout layout(char *base, int B, int T, int S, int reach_left, int reach_right) {
    Layout l;
    static_cast<Band &>(l) = band_of(S, reach_left, reach_right);
    Scratch a(base);
    l.Df = a.take<float>((size_t)l.W * l.Sd);
    l.Db = a.take<float>((size_t)l.W * l.Sd);
    l.m = a.take<float>((size_t)B * T);
    l.c = a.take<float>((size_t)B * T);
    l.flag = a.take<int32_t>(1);
    l.total = a.bytes + 256;                 // (room to align the caller's base)
    return l;
}

// LDS of a tile of G items: the rows [2][G][S + 2 halo] and the wave sums [2][G][16] fp32, the fp64 wave sums of L
// [G][16] and L [G]
__host__ __device__ inline int row_stride(int S, int halo) { return S + 2 * halo; }
inline size_t lds_bytes(int G, int S, int halo) {
    return (size_t)G * ((size_t)2 * row_stride(S, halo) * 4 + 2 * kWaves * 4 + kWaves * 8 + 8) + 16;
}

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}
// the 16 wave sums of one item (lane l holds number l & 15): every lane gets the same bits
__device__ __forceinline__ float sum16(float x) {
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// ---- the diagonals of E - ebg in both orders; resets the promise flag ----
__global__ void fb_band_prepare_kernel(const float *__restrict__ A, float *__restrict__ Df, float *__restrict__ Db,
                                       int32_t *__restrict__ flag, float ebg, int reach_left, int W, int Sd, int S) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *flag = 0;
    const size_t n = (size_t)W * Sd;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(e / Sd), x = (int)(e % Sd);
        const int i = x - reach_left + k;            // forward: x is the next state, i the prev state
        const int j = x + reach_left - k;            // backward: x is the prev state, j the next state
        Df[e] = (x < S && i >= 0 && i < S) ? expf(A[(size_t)x * S + i]) - ebg : 0.f;
        Db[e] = (x < S && j >= 0 && j < S) ? expf(A[(size_t)j * S + x]) - ebg : 0.f;
    }
}

// ---- the promise: every entry outside the band equals `background` bit for bit (band_diagonals.hpp); one wave per matrix row ----
__global__ __launch_bounds__(64) void fb_band_verify_kernel(const float *__restrict__ A, int32_t *__restrict__ flag,
                                                            float background, int reach_left, int reach_right, int S) {
    const int j = blockIdx.x, lane = threadIdx.x;
    if (banddiag::stray_in_row(A + (size_t)j * S, j, reach_left, reach_right, S, __float_as_uint(background), lane, 64)) *flag = 1;
}

// host: the two launches above, in this order -- what every band entry and the streaming prepare do to a matrix first
inline hipError_t prepare_and_verify(const float *A, const Band &b, float *Df, float *Db, int32_t *flag, float ebg,
                                     float background, int S, hipStream_t st) {
    const size_t cells = (size_t)b.W * b.Sd;
    hipLaunchKernelGGL(fb_band_prepare_kernel, dim3((unsigned)std::min<size_t>((cells + 255) / 256, 4096)), dim3(256), 0, st, A,
                       Df, Db, flag, ebg, b.reach_left, b.W, b.Sd, S);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fb_band_verify_kernel, dim3(S), dim3(64), 0, st, A, flag, background, b.reach_left, b.reach_right, S);
    return hipGetLastError();
}

// diagonal loads in flight per band sum of a tile of G items
constexpr int band_unroll(int G) { return G <= 2 ? 8 : (G <= 4 ? 4 : 2); }

// ---- the pieces fb_band_kernel, fb_band_counts_kernel (counts_band.hpp) and fb_band_filter_kernel (sample_band.hpp) share:
// this one definition of the ownership, the reductions and the order of the arithmetic fixes the bits of a_t, c_t and L of
// all three ----

// One tile of G items in the dynamic LDS of a workgroup (lds_bytes above), and the frames of its items.
template <int G>
struct Tile {
    double *lsum, *Ls;                       // [G][16] wave sums of L; [G] L as the float the caller gets
    float *rows, *part;                      // [2][G][stride]; [2][G][16] wave sums of a row
    int halo, stride, b0, Fmax, F[G];

    __device__ __forceinline__ Tile(unsigned char *lds, int reach_left, int reach_right, int S) {
        halo = reach_left > reach_right ? reach_left : reach_right;
        stride = row_stride(S, halo);
        lsum = reinterpret_cast<double *>(lds);
        Ls = lsum + G * kWaves;
        rows = reinterpret_cast<float *>(Ls + G);
        part = rows + (size_t)2 * G * stride;
    }
};

// items b0 .. b0 + G - 1: their frames, and zero rows (no barrier: the caller's next one covers the rows)
template <int G>
__device__ __forceinline__ void tile_begin(Tile<G> &tile, const int32_t *__restrict__ frames, int b0, int B, int T) {
    tile.b0 = b0;
    tile.Fmax = 1;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        tile.F[g] = b0 + g < B ? fb::frames_of(frames, b0 + g, T) : 0;  // (0: an item beyond the batch never takes a step)
        tile.Fmax = tile.F[g] > tile.Fmax ? tile.F[g] : tile.Fmax;
    }
    for (int e = threadIdx.x; e < 2 * G * tile.stride; e += kThreads) tile.rows[e] = 0.f;  // (the halos stay zero all tile long)
}

// rows an item does not have
template <int G>
__device__ __forceinline__ void zero_absent_rows(const Tile<G> &tile, float *__restrict__ post, int B, int T, int S) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (tile.b0 + g >= B) continue;
        float *out = post + (size_t)(tile.b0 + g) * T * S;
        for (size_t e = (size_t)tile.F[g] * S + threadIdx.x; e < (size_t)T * S; e += kThreads) out[e] = 0.f;
    }
}

// c_t of every item of the tile from the wave sums of frame t; thread 0 stores it for the later passes and L
template <int G>
__device__ __forceinline__ void row_sums(const Tile<G> &tile, int t, float *__restrict__ cbuf, int T, float *c) {
    const float *p = tile.part + (size_t)(t & 1) * G * kWaves;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        c[g] = sum16(p[g * kWaves + (threadIdx.x & 15)]);
        if (threadIdx.x == 0 && t < tile.F[g]) cbuf[(size_t)(tile.b0 + g) * T + t] = c[g];
    }
}

// ---- forward: a_0 = exp(pi + o_0 - m_0), a_t = e_t * (E a_{t-1}) / c_{t-1}; a_t to `out` [B][T][S], c_t to cbuf; ends
// behind a barrier, with every c_t of the tile stored ----
template <int G>
__device__ __forceinline__ void forward_pass(const Tile<G> &tile, const float *__restrict__ obs,
                                             const float *__restrict__ initial, const float *__restrict__ Df,
                                             const float *__restrict__ m, float *__restrict__ cbuf, float *__restrict__ out,
                                             float ebg, int reach_left, int W, int Sd, int T, int S) {
    constexpr int kUnroll = band_unroll(G);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int halo = tile.halo, stride = tile.stride, b0 = tile.b0;
    for (int t = 0; t < tile.Fmax; ++t) {
        float *cur = tile.rows + (size_t)(t & 1) * G * stride;
        const float *prev = tile.rows + (size_t)((t & 1) ^ 1) * G * stride;
        float cprev[G], acc[G];
        if (t > 0) row_sums(tile, t - 1, cbuf, T, cprev);
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = 0.f;
        float mt[G];
#pragma unroll
        for (int g = 0; g < G; ++g) mt[g] = t < tile.F[g] ? m[(size_t)(b0 + g) * T + t] : 0.f;
        for (int j = tid; j < S; j += kThreads) {
            float s[G], ot[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                s[g] = 0.f;
                ot[g] = t < tile.F[g] ? obs[((size_t)(b0 + g) * T + t) * S + j] : 0.f;    // (in flight during the band sum)
            }
            if (t > 0) {
                const float *d = Df + j;
                const float *x = prev + halo - reach_left + j;
#pragma unroll kUnroll
                for (int k = 0; k < W; ++k) {
                    const float dk = d[(size_t)k * Sd];
#pragma unroll
                    for (int g = 0; g < G; ++g) s[g] = fmaf(dk, x[g * stride + k], s[g]);
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t >= tile.F[g]) continue;
                const size_t row = (size_t)(b0 + g) * T + t;
                const float o = ot[g], mm = mt[g];
                float v;
                if (t == 0) {
                    v = expf(initial[j] + o - mm);
                } else {
                    const float e = expf(o - mm), c = cprev[g];
                    const float u = e * (ebg != 0.f ? fmaf(ebg, c, s[g]) : s[g]);
                    v = c == 0.f ? u * 0.f : u / c;                      // (after a zero-probability frame: 0, or NaN from NaN)
                }
                cur[g * stride + halo + j] = v;
                out[row * S + j] = v;
                acc[g] += v;
            }
        }
        float *p = tile.part + (size_t)(t & 1) * G * kWaves;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float a = wave_sum(acc[g]);
            if (lane == 0) p[g * kWaves + wave] = a;
        }
        __syncthreads();
    }
    {
        float c[G];
        row_sums(tile, tile.Fmax - 1, cbuf, T, c);
    }
    __syncthreads();                                                     // (c_t written by thread 0 is read by all below)
}

// ---- L = sum_{t<F} (log c_t + m_t) in fp64; NaN when the sum is NaN or +inf, or the promise is broken.  To loglik and, as
// the float the caller gets, to tile.Ls: a caller that reads Ls puts a barrier in front ----
template <int G>
__device__ __forceinline__ void log_likelihood(const Tile<G> &tile, const float *__restrict__ m, const float *__restrict__ cbuf,
                                               const int32_t *__restrict__ flag, float *__restrict__ loglik, int B, int T) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        double a = 0.;
        for (int t = tid; t < tile.F[g]; t += kThreads) {
            const size_t row = (size_t)(tile.b0 + g) * T + t;
            a += log((double)cbuf[row]) + (double)m[row];
        }
        a = wave_sum(a);
        if (lane == 0) tile.lsum[g * kWaves + wave] = a;
    }
    __syncthreads();
    if (tid < G) {
        double L = 0.;
        for (int w = 0; w < kWaves; ++w) L += tile.lsum[tid * kWaves + w];
        float out = (L != L || L == (double)INFINITY) ? NAN : (float)L;
        if (*flag != 0) out = NAN;
        tile.Ls[tid] = (double)out;
        if (tile.b0 + tid < B) loglik[tile.b0 + tid] = out;
    }
}

// ---- both passes of G items per workgroup; grid ceil(B / G), dynamic LDS lds_bytes(G, S, halo) ----
template <int G>
__global__ __launch_bounds__(kThreads) void fb_band_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                           const float *__restrict__ initial, const float *__restrict__ Df,
                                                           const float *__restrict__ Db, const float *__restrict__ m,
                                                           float *__restrict__ cbuf, const int32_t *__restrict__ flag,
                                                           float *__restrict__ post, float *__restrict__ loglik, float ebg,
                                                           int reach_left, int reach_right, int W, int Sd, int B, int T,
                                                           int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Tile<G> tile(lds_raw, reach_left, reach_right, S);
    tile_begin(tile, frames, blockIdx.x * G, B, T);
    zero_absent_rows(tile, post, B, T, S);
    __syncthreads();
    forward_pass(tile, obs, initial, Df, m, cbuf, post, ebg, reach_left, W, Sd, T, S);
    log_likelihood(tile, m, cbuf, flag, loglik, B, T);
    __syncthreads();

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int halo = tile.halo, stride = tile.stride, b0 = tile.b0, Fmax = tile.Fmax;
    const int *F = tile.F;
    float *const rows = tile.rows, *const part = tile.part;
    const double *Ls = tile.Ls;
    constexpr int kUnroll = band_unroll(G);
    bool bad[G];
#pragma unroll
    for (int g = 0; g < G; ++g) bad[g] = !isfinite(Ls[g]);

    // ---- backward: b_{F-1} = 1, b_t = E^T w_{t+1}; gamma_t = a_t b_t / c_t in place, w_t = e_t b_t / c_t ----
    for (int t = Fmax - 1; t >= 0; --t) {
        float *cur = rows + (size_t)(t & 1) * G * stride;
        const float *prev = rows + (size_t)((t & 1) ^ 1) * G * stride;
        const bool step = t < Fmax - 1;
        float sw[G], acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) sw[g] = acc[g] = 0.f;
        if (ebg != 0.f && step) {
            const float *p = part + (size_t)((t & 1) ^ 1) * G * kWaves;
#pragma unroll
            for (int g = 0; g < G; ++g) sw[g] = sum16(p[g * kWaves + (lane & 15)]);
        }
        float mt[G], ct[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            mt[g] = t < F[g] ? m[(size_t)(b0 + g) * T + t] : 0.f;
            ct[g] = t < F[g] ? cbuf[(size_t)(b0 + g) * T + t] : 1.f;
        }
        for (int j = tid; j < S; j += kThreads) {
            float s[G], ot[G], at[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                s[g] = 0.f;
                const size_t at_j = ((size_t)(b0 + g) * T + t) * S + j;
                ot[g] = t < F[g] ? obs[at_j] : 0.f;                      // (in flight during the band sum)
                at[g] = t < F[g] ? post[at_j] : 0.f;
            }
            if (step) {
                const float *d = Db + j;
                const float *x = prev + halo + reach_left + j;
#pragma unroll kUnroll
                for (int k = 0; k < W; ++k) {
                    const float dk = d[(size_t)k * Sd];
#pragma unroll
                    for (int g = 0; g < G; ++g) s[g] = fmaf(dk, x[g * stride - k], s[g]);
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t >= F[g]) continue;
                const size_t row = (size_t)(b0 + g) * T + t;
                const float o = ot[g], mm = mt[g], c = ct[g], a = at[g];
                const float beta = t == F[g] - 1 ? 1.f : (ebg != 0.f ? fmaf(ebg, sw[g], s[g]) : s[g]);
                const float w = (expf(o - mm) * beta) / c;              // (w_0 is never read)
                post[row * S + j] = bad[g] ? NAN : (a * beta) / c;
                cur[g * stride + halo + j] = w;
                acc[g] += w;
            }
        }
        if (ebg != 0.f) {
            float *p = part + (size_t)(t & 1) * G * kWaves;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float a = wave_sum(acc[g]);
                if (lane == 0) p[g * kWaves + wave] = a;
            }
        }
        __syncthreads();
    }
}

}  // namespace fbb
