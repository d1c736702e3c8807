// path_entropy_band.hpp -- path entropy for a transition matrix that holds ONE value outside a band
// (torbi_hip_path_entropy_band, torbi_amd/entropy.py forward_entropy_banded, ENTROPY.md "Band route").
//
// The model, the contract and the recursion are path_entropy.hpp's; the band, the background and the promise about the
// entries outside the band are forward_backward_band.hpp's.  With ebg = exp(background) and gbg = ebg * background (both 0
// for -inf: 0 x -inf is never formed), E = exp(A), G = E o A (0 where A = -inf, inside the band too):
//     Df[k][j] = E[j][j - reach_left + k] - ebg        Dg[k][j] = G[j][j - reach_left + k] - gbg        (0 where clipped)
// every product of the recursion splits into the band and one constant, 3 W multiplies per state where the dense route
// spends 3 S.
//
// The division by c_t is deferred.  With the row the scaled forward pass carries anyway, a_t = e_t * d_t (sum_j a_t[j] = c_t,
// p_t = a_t / c_t), and v_t = a_t h_t - xlogx(a_t):
//     u_t = (v_t + a_t log c_t) / c_t            prefix_t = (sum_j v_t[j]) / c_t + log c_t
//     d  = (Df a) / c + ebg                                                                 (a, v, c of frame t - 1)
//     D2 = (Df v + log c * Df a) / c + ebg * prefix_{t-1}            D3 = (Dg a) / c + gbg
//     h_t[j] = log d + (D2 - D3) / d     (0 where d = 0)             a_t[j] = e_t[j] d[j]
// so a frame is ONE band sweep over the pair (a, v) and one barrier: the structure of fbb::forward_pass, with the same c_t.
// The three sums are divided by c BEFORE the constants join them: d then never falls below ebg, as on the dense route.  (With
// Sa = Df a + ebg c, h = log Sa + (Sv - Sg) / Sa is the same number without log c, but where float32 underflows inside the
// band a state lives on the background alone, ebg c is a denormal for c < 1, and its lost bits showed in H: 19.4 units of
// 1e-6 |H| + 1e-6 F at 2 x 500 x 200 with log(tiny) outside, against 3.7 in this form.)  A single-path model gives
// -xlogx(a) / c + log c with c == a, which is 0 only within rounding: this route promises the bound, not exact zeros.
//
// Workspace (torbi_hip_path_entropy_band_workspace_size), every piece 256-B aligned, Sd = S up to 64:
//     Df, Dg  2 x [W][Sd] fp32
//     m, c    2 x [B][T]  fp32   row maxima (fb_rowmax_kernel), row sums c_t
//     prefix  [B][T]      fp32   (the caller's prefix output takes its place where there is one)
//     flag    int32              1 when an entry outside the stated band differs from `background`
// No (B, T, S) piece; every word that is read was written by the same call.
//
// pe_band_kernel<G>: ONE launch runs all T frames.  A workgroup of 1024 threads owns G whole items, so nothing waits across
// workgroups; thread `tid` owns states tid, tid + 1024, ...  The pairs (a_t[i], v_t[i]) of the tile live in LDS as one 8-byte
// element, by parity of t, with a zero halo of max(reach) on both sides; both diagonal sets stream from L2 and every load
// of one is shared by the G items.
//
// Reductions, per item and in a fixed order that does not depend on G: c_t in fp32 as fbb (a 64-lane butterfly per wave, the
// 16 wave sums by a 16-lane butterfly); sum_j v_t[j] in fp64 the same way (a thread's states in order first); prefix_t in
// fp64 from the two, rounded once; L by fbb::log_likelihood.  No float atomics, vector stores only.
#pragma once

#include "forward_backward_band.hpp"
#include "path_entropy.hpp"

namespace peb {

using fbb::kThreads;
using fbb::kWaves;

constexpr int kMaxStates = fbb::kMaxStates;
constexpr int kMaxWindow = fbb::kMaxWindow;
constexpr int kMaxGroup = 4;                 // items per workgroup (8, at three sums per item, would not fit 128 VGPRs without scratch)
// The LDS budget: 159 of the 160 KB of a compute unit.  A workgroup of 1024 threads above 64 VGPRs is alone on its compute
// unit whatever its LDS, so the rows may take it all: 1440 states at reach 11 / 11 put 4 items there (23.9 KB each), and the
// largest covered row (4096 states, reach 63) fits once (67.9 KB), so the budget refuses no shape the window admits.
constexpr int kMaxLdsBytes = 159 * 1024;

struct Layout : fbb::Band { float *Df, *Dg, *m, *c, *prefix; int32_t *flag; size_t total; };

// `base`: the caller's workspace aligned up to 256 bytes, or null for the byte count alone
inline Layout layout(char *base, int B, int T, int S, int reach_left, int reach_right) {
    Layout l;
    static_cast<fbb::Band &>(l) = fbb::band_of(S, reach_left, reach_right);
    Scratch a(base);
    l.Df = a.take<float>((size_t)l.W * l.Sd);
    l.Dg = a.take<float>((size_t)l.W * l.Sd);
    l.m = a.take<float>((size_t)B * T);
    l.c = a.take<float>((size_t)B * T);
    l.prefix = a.take<float>((size_t)B * T);
    l.flag = a.take<int32_t>(1);
    l.total = a.bytes + 256;                 // (room to align the caller's base)
    return l;
}

// LDS of a tile of G items: fbb::Tile's head (the fp64 wave sums of L [G][16] and L [G]), the pairs [2][G][S + 2 halo] of
// 8 bytes, the fp64 wave sums of v [2][G][16], the fp32 wave sums of a [2][G][16] and H [G]
inline size_t lds_bytes(int G, int S, int halo) {
    return (size_t)G * (kWaves * 8 + 8 + (size_t)2 * fbb::row_stride(S, halo) * 8 + 2 * kWaves * 8 + 2 * kWaves * 4 + 4) + 16;
}

// the 16 fp64 wave sums of one item (lane l holds number l & 15): every lane gets the same bits
__device__ __forceinline__ double sum16(double x) {
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// ---- the diagonals of E - ebg and of G - gbg along the next state; resets the promise flag ----
__global__ void pe_band_prepare_kernel(const float *__restrict__ A, float *__restrict__ Df, float *__restrict__ Dg,
                                       int32_t *__restrict__ flag, float ebg, float gbg, int reach_left, int W, int Sd, int S) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *flag = 0;
    const size_t n = (size_t)W * Sd;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(e / Sd), j = (int)(e % Sd);
        const int i = j - reach_left + k;
        float f = 0.f, g = 0.f;
        if (j < S && i >= 0 && i < S) {
            const float a = A[(size_t)j * S + i], x = expf(a);
            f = x - ebg;
            g = (a == -INFINITY ? 0.f : x * a) - gbg;
        }
        Df[e] = f;
        Dg[e] = g;
    }
}

// host: the diagonals, then fbb's check of the promise (which sets the flag the launch above reset)
inline hipError_t prepare_and_verify(const float *A, const Layout &l, float ebg, float gbg, float background, int S,
                                     hipStream_t st) {
    const size_t cells = (size_t)l.W * l.Sd;
    hipLaunchKernelGGL(pe_band_prepare_kernel, dim3((unsigned)std::min<size_t>((cells + 255) / 256, 4096)), dim3(256), 0, st, A,
                       l.Df, l.Dg, l.flag, ebg, gbg, l.reach_left, l.W, l.Sd, S);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fbb::fb_band_verify_kernel, dim3(S), dim3(64), 0, st, A, l.flag, background, l.reach_left, l.reach_right,
                       S);
    return hipGetLastError();
}

// fbb's tile (the frames of the items, the fp64 sums of L) with the rows as pairs and the sums of both halves of a pair
template <int G>
struct Tile : fbb::Tile<G> {
    float2 *pairs;                           // [2][G][stride]: (a_t[i], v_t[i]) at halo + i
    double *vsum;                            // [2][G][16] wave sums of v_t
    float *asum, *Hs;                        // [2][G][16] wave sums of a_t; [G] prefix_{F-1}

    __device__ __forceinline__ Tile(unsigned char *lds, int reach_left, int reach_right, int S)
        : fbb::Tile<G>(lds, reach_left, reach_right, S) {
        pairs = reinterpret_cast<float2 *>(this->rows);                  // (behind lsum and Ls: 8-byte aligned)
        vsum = reinterpret_cast<double *>(pairs + (size_t)2 * G * this->stride);
        asum = reinterpret_cast<float *>(vsum + 2 * G * kWaves);
        Hs = asum + 2 * G * kWaves;
    }
};

// c_t and sum_j v_t[j] of every item of the tile from the wave sums of frame t (every thread, the same bits); lane 0 of
// wave g stores c_t and prefix_t of item g, and keeps prefix_{F-1} for the end
template <int G>
__device__ __forceinline__ void frame_sums(const Tile<G> &tile, int t, float *__restrict__ cbuf, float *__restrict__ prefix,
                                           int T, float *c, float *sv) {
    const float *pa = tile.asum + (size_t)(t & 1) * G * kWaves;
    const double *pv = tile.vsum + (size_t)(t & 1) * G * kWaves;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        c[g] = fbb::sum16(pa[g * kWaves + (threadIdx.x & 15)]);
        const double v = sum16(pv[g * kWaves + (threadIdx.x & 15)]);
        sv[g] = (float)v;
        if (threadIdx.x == g * 64 && t < tile.F[g]) {
            const size_t row = (size_t)(tile.b0 + g) * T + t;
            const float h = (float)(v / (double)c[g] + log((double)c[g]));
            cbuf[row] = c[g];
            prefix[row] = h;
            if (t == tile.F[g] - 1) tile.Hs[g] = h;
        }
    }
}

// ---- every frame of G items per workgroup; grid ceil(B / G), dynamic LDS lds_bytes(G, S, halo) ----
template <int G>
__global__ __launch_bounds__(kThreads) void pe_band_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                           const float *__restrict__ initial, const float *__restrict__ Df,
                                                           const float *__restrict__ Dg, const float *__restrict__ m,
                                                           float *__restrict__ cbuf, const int32_t *__restrict__ flag,
                                                           float *__restrict__ prefix, float *__restrict__ entropy,
                                                           float *__restrict__ loglik, float ebg, float gbg, int reach_left,
                                                           int reach_right, int W, int Sd, int B, int T, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Tile<G> tile(lds_raw, reach_left, reach_right, S);
    fbb::tile_begin(tile, frames, blockIdx.x * G, B, T);                // (zeroes the first half of the pairs)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int halo = tile.halo, stride = tile.stride, b0 = tile.b0;
    for (int e = 2 * G * stride + tid; e < 4 * G * stride; e += kThreads) tile.rows[e] = 0.f;
    // prefix entries an item does not have
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (b0 + g >= B) continue;
        for (int t = tile.F[g] + tid; t < T; t += kThreads) prefix[(size_t)(b0 + g) * T + t] = 0.f;
    }
    __syncthreads();

    constexpr int kUnroll = fbb::band_unroll(G);
    for (int t = 0; t < tile.Fmax; ++t) {
        float2 *cur = tile.pairs + (size_t)(t & 1) * G * stride;
        const float2 *prev = tile.pairs + (size_t)((t & 1) ^ 1) * G * stride;
        float rc[G], logc[G], eb[G], gb[G], ep[G], acc[G], mt[G];
        double vacc[G];
        if (t > 0) {
            float cprev[G], svprev[G];
            frame_sums(tile, t - 1, cbuf, prefix, T, cprev, svprev);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                // (after a zero-probability frame: every a_t is 0, or NaN from NaN, and the background brings nothing back)
                const bool dead = cprev[g] == 0.f;
                rc[g] = dead ? 0.f : 1.f / cprev[g];
                logc[g] = dead ? 0.f : logf(cprev[g]);
                eb[g] = dead ? 0.f : ebg;
                gb[g] = dead ? 0.f : gbg;
                ep[g] = ebg != 0.f ? eb[g] * fmaf(svprev[g], rc[g], logc[g]) : 0.f;    // ebg * sum_i u[i] = ebg * prefix_{t-1}
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            acc[g] = 0.f;
            vacc[g] = 0.;
            mt[g] = t < tile.F[g] ? m[(size_t)(b0 + g) * T + t] : 0.f;
        }
        for (int j = tid; j < S; j += kThreads) {
            float sa[G], sv[G], sg[G], ot[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                sa[g] = sv[g] = sg[g] = 0.f;
                ot[g] = t < tile.F[g] ? obs[((size_t)(b0 + g) * T + t) * S + j] : 0.f;    // (in flight during the band sums)
            }
            if (t > 0) {
                const float *df = Df + j, *dg = Dg + j;
                const float2 *x = prev + halo - reach_left + j;
#pragma unroll kUnroll
                for (int k = 0; k < W; ++k) {
                    const float fk = df[(size_t)k * Sd], gk = dg[(size_t)k * Sd];
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const float2 av = x[g * stride + k];
                        sa[g] = fmaf(fk, av.x, sa[g]);
                        sv[g] = fmaf(fk, av.y, sv[g]);
                        sg[g] = fmaf(gk, av.x, sg[g]);
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t >= tile.F[g]) continue;
                float a, h = 0.f;
                if (t == 0) {
                    a = expf(initial[j] + ot[g] - mt[g]);
                } else {
                    // d = E p, D2 = E u and D3 = G p of the normalised rows, each the band over c_{t-1} plus its constant
                    const float d = fmaf(sa[g], rc[g], eb[g]);
                    const float D2 = fmaf(fmaf(logc[g], sa[g], sv[g]), rc[g], ep[g]);
                    const float D3 = fmaf(sg[g], rc[g], gb[g]);
                    a = expf(ot[g] - mt[g]) * d;
                    if (d > 0.f) h = logf(d) + (D2 - D3) / d;            // (0 where no path reaches j)
                }
                const float v = a * h - pe::xlogx(a);
                cur[g * stride + halo + j] = make_float2(a, v);
                acc[g] += a;
                vacc[g] += (double)v;
            }
        }
        float *pa = tile.asum + (size_t)(t & 1) * G * kWaves;
        double *pv = tile.vsum + (size_t)(t & 1) * G * kWaves;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float a = fbb::wave_sum(acc[g]);
            const double v = fbb::wave_sum(vacc[g]);
            if (lane == 0) {
                pa[g * kWaves + wave] = a;
                pv[g * kWaves + wave] = v;
            }
        }
        __syncthreads();
    }
    {
        float c[G], sv[G];
        frame_sums(tile, tile.Fmax - 1, cbuf, prefix, T, c, sv);
    }
    __syncthreads();                                                     // (c_t, prefix_t and Hs are read by others below)
    fbb::log_likelihood(tile, m, cbuf, flag, loglik, B, T);
    __syncthreads();
    // an item whose L is not finite (or a broken promise: L is NaN then): a NaN entropy and NaN in its prefix entries t < F
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (b0 + g >= B) continue;
        const bool bad = !isfinite(tile.Ls[g]);
        if (tid == 0) entropy[b0 + g] = bad ? NAN : tile.Hs[g];
        if (!bad) continue;
        for (int t = tid; t < tile.F[g]; t += kThreads) prefix[(size_t)(b0 + g) * T + t] = NAN;
    }
}

}  // namespace peb
