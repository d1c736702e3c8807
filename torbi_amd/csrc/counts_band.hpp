// counts_band.hpp -- expected transition counts on a band (torbi_hip_forward_backward_counts_band, torbi_amd/training.py
// forward_backward_counts_banded, POSTERIOR.md "Band counts").
//
// The contract is counts.hpp's, the model and the passes are forward_backward_band.hpp's:
//     X = E (.) sum_b g_b sum_{t=1}^{F_b-1} w_t^b (x) (a_{t-1}^b / c_{t-1}^b)
// Backward iteration t of fb_band_kernel has everything pair t + 1 needs in the thread that owns prev state i: a_t[i] and
// c_t in registers, and its band sum already reads w_{t+1}[i + reach_left - k] from the LDS row for every diagonal k.  So
//     Cb[k][i] += sum_g q_g w_{t+1}^g[i + reach_left - k]        q_g = g_b a_t^g[i] / c_t^g
// costs one more multiply-add per LDS value that is read anyway.  Cb has Db's layout (diagonal k along the prev state) and
// lives in LDS, one fp32 plane [W][S] per workgroup behind the rows: only the owning thread ever touches a cell, consecutive
// threads hit consecutive banks, no barrier and no LDS row is added.  (Accumulators in registers spill at every shape that
// was compiled: HISTORY.md.)
//
// fb_band_counts_kernel<G> is fb_band_kernel<G> with that accumulation and a persistent loop over tiles: the grid is
// min(tiles, kCountsWorkgroups), workgroup p takes tiles p, p + grid, ... and stores its plane to partial[p] at the end.  It is
// a second kernel, not a flag of the first, so that the posterior route keeps its instances as they are; the forward pass and
// L are fb_band_kernel's own functions (forward_pass, log_likelihood), the backward pass is written out here with the same
// ownership, butterflies and order, so gamma, c_t and L of an item are bit for bit fb_band_kernel's.
// fb_band_counts_finalize_kernel sums the planes in order, multiplies by exp(A) and turns the diagonals to the forward layout.
//
// An item counts iff g_b != 0 and its L_b is finite (known before the backward pass).  One that does not, or a frame behind
// an item's last pair, is skipped by selection: q_g and the LDS value are both selected to 0, never multiplied by 0 (the row
// of such an item may hold NaN).  The order is fixed -- items of the tile in order within a frame, frames from F - 2 down to
// 0, tiles in the workgroup's order, planes in order --, so the bits depend on the inputs and the tile size only.  No float
// atomics, nothing waits across workgroups, vector stores only.
#pragma once

#include <type_traits>

#include "counts.hpp"
#include "forward_backward_band.hpp"

namespace fbb {

constexpr int kCountsWorkgroups = 512;       // P: planes of a call (a compile-time constant: the workspace needs no device)
constexpr int kCountsLdsBytes = 160 * 1024;  // rows and plane of one workgroup: the LDS of a compute unit

inline size_t plane_bytes(int W, int S) { return (size_t)4 * W * S; }

struct CountsLayout : Layout {
    float *partial;                          // [planes][W][Sd] fp32
    int planes;                              // min(B, kCountsWorkgroups): no call has more workgroups
};

// the band route's workspace, then the planes
inline CountsLayout counts_layout(char *base, int B, int T, int S, int reach_left, int reach_right) {
    CountsLayout l;
    static_cast<Layout &>(l) = layout(base, B, T, S, reach_left, reach_right);
    Scratch a(base, l.total - 256);
    l.planes = B < kCountsWorkgroups ? B : kCountsWorkgroups;
    l.partial = a.take<float>((size_t)l.planes * l.W * l.Sd);
    l.total = a.bytes + 256;
    return l;
}

// a value every lane of the wave holds, moved to a scalar register (the kernel has 128 vector registers and none to spare)
__device__ __forceinline__ float wave_uniform(float x) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

// ---- both passes and the counts of G items per tile; grid min(tiles, kCountsWorkgroups), dynamic LDS lds_bytes(G, S, halo)
// + plane_bytes(W, S) ----
// (waves per SIMD: every instance needs more than 64 vector registers, so a compute unit holds one workgroup, four waves per
// SIMD, whatever else the count is.  Left to itself the compiler plans G = 2 for six waves, 80 registers, and pays with the
// forward band sum's loads in flight: one at a time, 8 % of the call at 512 x 500 x 1440.  "At most five" leaves it 96.
// "At most four" is the plain truth and compiles the same sum worse at G = 2 and G = 4: HISTORY.md)
template <int G>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 5))) void fb_band_counts_kernel(
    const float *__restrict__ obs, const int32_t *__restrict__ frames, const float *__restrict__ initial,
    const float *__restrict__ Df, const float *__restrict__ Db, const float *__restrict__ m, float *__restrict__ cbuf,
    const int32_t *__restrict__ flag, const float *__restrict__ weights, float *__restrict__ post, float *__restrict__ loglik,
    float *__restrict__ partial, float ebg, int reach_left, int reach_right, int W, int Sd, int B, int T, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Tile<G> tile(lds_raw, reach_left, reach_right, S);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int halo = tile.halo, stride = tile.stride;
    const int *F = tile.F;
    float *const rows = tile.rows, *const part = tile.part;
    const double *Ls = tile.Ls;
    float *plane = part + 2 * G * kWaves;                                // [W][S]: Cb of this workgroup
    constexpr bool kLateObs = G >= 8;       // o_t is loaded behind the band sum, not during it: 8 registers the sum needs
    constexpr int kBatch = G <= 2 ? 4 : (G <= 4 ? 2 : 1);  // diagonals whose LDS loads go out before the plane's stores

    for (int k = 0; k < W; ++k)                                          // (by the owner, like every later access: no barrier)
        for (int i = tid; i < S; i += kThreads) plane[(size_t)k * S + i] = 0.f;

    const int tiles = (B + G - 1) / G;
    for (int t0 = blockIdx.x; t0 < tiles; t0 += gridDim.x) {
        tile_begin(tile, frames, t0 * G, B, T);
        zero_absent_rows(tile, post, B, T, S);
        __syncthreads();
        forward_pass(tile, obs, initial, Df, m, cbuf, post, ebg, reach_left, W, Sd, T, S);
        log_likelihood(tile, m, cbuf, flag, loglik, B, T);
        __syncthreads();
        const int b0 = tile.b0, Fmax = tile.Fmax;
        bool bad[G];
        float gw[G];                                                     // g_b of an item that counts, else 0
#pragma unroll
        for (int g = 0; g < G; ++g) {
            bad[g] = !isfinite(Ls[g]);
            const float gb = b0 + g < B ? (weights ? weights[b0 + g] : 1.f) : 0.f;
            gw[g] = wave_uniform(bad[g] ? 0.f : gb);
        }

        // ---- backward: b_{F-1} = 1, b_t = E^T w_{t+1}; gamma_t = a_t b_t / c_t in place, w_t = e_t b_t / c_t; pair t + 1 ----
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
                for (int g = 0; g < G; ++g) sw[g] = wave_uniform(sum16(p[g * kWaves + (lane & 15)]));
            }
            float mt[G], ct[G], gc[G];
            bool use[G], all_use = true;                                 // item g has pair t + 1 and counts
#pragma unroll
            for (int g = 0; g < G; ++g) {
                mt[g] = wave_uniform(t < F[g] ? m[(size_t)(b0 + g) * T + t] : 0.f);
                ct[g] = wave_uniform(t < F[g] ? cbuf[(size_t)(b0 + g) * T + t] : 1.f);
                use[g] = t + 1 < F[g] && gw[g] != 0.f;
                gc[g] = wave_uniform(use[g] ? gw[g] / ct[g] : 0.f);
                all_use = all_use && use[g];
            }
            for (int j = tid; j < S; j += kThreads) {
                float s[G], ot[G], at[G], q[G];
                auto load_obs = [&]() {
#pragma unroll
                    for (int g = 0; g < G; ++g) ot[g] = t < F[g] ? obs[((size_t)(b0 + g) * T + t) * S + j] : 0.f;
                };
                if (!kLateObs) load_obs();                               // (in flight during the band sum)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    s[g] = 0.f;
                    at[g] = t < F[g] ? post[((size_t)(b0 + g) * T + t) * S + j] : 0.f;
                }
                if (step) {
                    const float *d = Db + j;
                    const float *x = prev + halo + reach_left + j;
                    float *cb = plane + j;
#pragma unroll
                    for (int g = 0; g < G; ++g) q[g] = use[g] ? at[g] * gc[g] : 0.f;
                    // kBatch diagonals at a time: every LDS load of the batch goes out before the first store to the plane
                    // (the compiler cannot tell that a store to the plane leaves the rows alone).  select: some item of the
                    // tile has no pair here, so its LDS value is selected to 0 beside its q
                    auto band_sum = [&](auto select) {
                        for (int k0 = 0; k0 < W; k0 += kBatch) {
                            float dk[kBatch], xv[kBatch][G], pv[kBatch];
#pragma unroll
                            for (int kk = 0; kk < kBatch; ++kk) {
                                const int k = k0 + kk < W ? k0 + kk : W - 1;     // (a batch past the last diagonal reads it again)
                                dk[kk] = d[(size_t)k * Sd];
                                pv[kk] = cb[(size_t)k * S];
#pragma unroll
                                for (int g = 0; g < G; ++g) xv[kk][g] = x[g * stride - k];
                            }
#pragma unroll
                            for (int kk = 0; kk < kBatch; ++kk) {
                                if (k0 + kk >= W) break;
                                float u = 0.f;
#pragma unroll
                                for (int g = 0; g < G; ++g) {
                                    s[g] = fmaf(dk[kk], xv[kk][g], s[g]);
                                    u = fmaf(q[g], decltype(select)::value && !use[g] ? 0.f : xv[kk][g], u);
                                }
                                cb[(size_t)(k0 + kk) * S] = pv[kk] + u;
                            }
                        }
                    };
                    if (all_use) band_sum(std::false_type()); else band_sum(std::true_type());
                }
                if (kLateObs) load_obs();
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (t >= F[g]) continue;
                    const size_t row = (size_t)(b0 + g) * T + t;
                    const float o = ot[g], mm = mt[g], c = ct[g], a = at[g];
                    const float beta = t == F[g] - 1 ? 1.f : (ebg != 0.f ? fmaf(ebg, sw[g], s[g]) : s[g]);
                    const float w = (expf(o - mm) * beta) / c;          // (w_0 is never read)
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

    // every cell of the plane is its owner's: nothing to wait for
    float *out = partial + (size_t)blockIdx.x * W * Sd;
    for (int k = 0; k < W; ++k)
        for (int i = tid; i < S; i += kThreads) out[(size_t)k * Sd + i] = plane[(size_t)k * S + i];
}

// ---- band_counts[k][j] = exp(A[j][i]) * sum_p partial[p][k][i], i = j - reach_left + k; 0 where the matrix clips the
// diagonal, NaN everywhere (the initial counts too) where the promise is broken ----
__global__ __launch_bounds__(256) void fb_band_counts_finalize_kernel(const float *__restrict__ A,
                                                                      const float *__restrict__ partial,
                                                                      const int32_t *__restrict__ flag,
                                                                      float *__restrict__ band_counts,
                                                                      float *__restrict__ initial_counts, int planes,
                                                                      int reach_left, int W, int Sd, int S) {
    const bool broken = *flag != 0;
    const size_t n = (size_t)W * S, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (broken && first < (size_t)S) initial_counts[first] = NAN;     // (the grid has at least S threads)
    for (size_t e = first; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(e / S), j = (int)(e % S);
        const int i = j - reach_left + k;
        float v = 0.f;
        if (i >= 0 && i < S) {
            float s = 0.f;
            const float *p = partial + (size_t)k * Sd + i;
            for (int q = 0; q < planes; ++q) s += p[(size_t)q * W * Sd];
            v = expf(A[(size_t)j * S + i]) * s;
        }
        band_counts[e] = broken ? NAN : v;
    }
}

}  // namespace fbb
