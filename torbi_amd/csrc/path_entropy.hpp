// path_entropy.hpp -- the entropy of the posterior over whole state paths (torbi_hip_path_entropy / _uniform,
// torbi_amd/entropy.py, ENTROPY.md).
//
//     H_b = - sum over every path q of item b of P(q | o_b) log P(q | o_b)      (nats)
//
// The forward-only recursion of Hernando, Crespi and Cybenko (2005) on the scaled forward pass of forward_backward.hpp.  With
// E = exp(A) ([next][prev]), G = E o A (0 where A = -inf: 0 x -inf is never formed), m_t = max_j o_t[j] (t = 0:
// max_j (pi + o_0)[j]), p_t the filtered distribution and xlogx(0) = 0:
//     a_0 = exp(pi + o_0 - m_0),  h_0 = 0
//     d = E p_{t-1},  D2 = E u_{t-1},  D3 = G p_{t-1}                          (three products, one launch)
//     a_t[j] = exp(o_t[j] - m_t) * d[j]
//     h_t[j] = log d[j] + (D2[j] - D3[j]) / d[j]                               (0 where d[j] = 0: no path reaches j)
//     c_t = sum_j a_t[j]   (32-row partials, then in order)     p_t = a_t / c_t
//     u_t[j] = p_t[j] h_t[j] - xlogx(p_t[j])                    prefix_t = sum_j u_t[j]   (fp64, rounded once)
//     L = sum_{t<F} (log c_t + m_t)   (fp64)                    H = prefix_{F-1}
// h_t[j] is the entropy of q_0 .. q_{t-1} given q_t = j; the observation at t cancels out of it.
//
// Per frame t >= 1: pe_step_kernel (the products on the f32 MFMA, v_mfma_f32_32x32x2_f32, over a 32 x 32 tile of states x
// items; a_t, h_t and the partial sums of a_t) and pe_item_kernel (a workgroup per item: c_t, p_t, u_t in place, prefix_t).
// Nothing waits across workgroups and nothing is allocated, so a call captures into a graph.  Output column n of an MFMA
// reads column n of the operands only, and every reduction over states runs per item in a fixed order: an item's bits do
// not depend on the other items.
//
// Workspace (torbi_hip_path_entropy_workspace_size), every piece 256-B aligned:
//     E, G     [Mp][Sp] fp32   rows >= S and columns >= S zero (Mp = S up to 64, Sp = S up to 32)
//     m, c     [B][T]   fp32   row maxima (-inf replaced by 0) and row sums
//     partial  [2][B][ceil(S/32)] fp32   per-32-row sums of a_t, by parity of t
//     p, u     [2][B][Sp] fp32 each      a_t then p_t, h_t then u_t, by parity of t; columns >= S of a live row are zero
//     prefix   [B][T]   fp32   (the caller's prefix output takes its place where there is one)
// Uniform route: rowh, lse [B][T] fp64, each row's entropy and log-sum-exp.  No piece grows as B T S.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "scratch.hpp"
#include "forward_backward.hpp"

namespace pe {

using fb::f32x4;
using fb::f32x16;
using fb::frames_of;
using fb::nan_max;
using fb::padded_rows;
using fb::padded_states;
using fb::partials_of;
using fb::sum32;

constexpr int kMaxStates = fb::kMaxStates;
constexpr int kStateTile = 32;               // rows of E and G per workgroup of a step launch
constexpr int kItemTile = 32;                // items per workgroup: one MFMA column each, for p and for u
constexpr int kMaxWaves = 4;                 // K is split over at most four waves (three 32 x 32 tiles each in LDS)
constexpr int kBlockK = 64, kLdsStride = 68; // staged form (68: the float4 operand reads of 16 rows cover all 64 banks once)
constexpr int kRowRegs = fb::kRowRegs;       // float4 per lane of a uniform-route row held in registers (S <= 2048)
constexpr int kStepLds = kMaxWaves * 3 * 1024;
static_assert(kStepLds >= 4 * 32 * kLdsStride, "the staging blocks fit where the reduction runs");

// Waves that split K in a step launch: a function of the states alone (every wave has at least one 8-wide chunk), so the
// order in which an item's products are summed does not depend on the batch.
__host__ __device__ inline int waves_of(int S) { return S >= 8 * kMaxWaves ? kMaxWaves : (S >= 16 ? 2 : 1); }

struct Layout {
    float *E, *G, *m, *c, *partial, *p, *u, *prefix;   // dense
    double *rowh, *lse;                                // uniform
    size_t total;
};

// `base`: the caller's workspace aligned up to 256 bytes, or null for the byte count alone
inline Layout layout(char *base, int B, int T, int S, bool uniform) {
    const size_t Sp = (size_t)padded_states(S), Mp = (size_t)padded_rows(S), BT = (size_t)B * T;
    Scratch a(base);
    Layout l{};
    if (uniform) {
        l.rowh = a.take<double>(BT);
        l.lse = a.take<double>(BT);
    } else {
        l.E = a.take<float>(Mp * Sp);
        l.G = a.take<float>(Mp * Sp);
        l.m = a.take<float>(BT);
        l.c = a.take<float>(BT);
        l.partial = a.take<float>((size_t)2 * B * partials_of(S));
        l.p = a.take<float>((size_t)2 * B * Sp);
        l.u = a.take<float>((size_t)2 * B * Sp);
        l.prefix = a.take<float>(BT);
    }
    l.total = a.bytes + 256;                 // (room to align the caller's base)
    return l;
}

__device__ __forceinline__ float xlogx(float p) { return p > 0.f ? p * logf(p) : 0.f; }

// ---- matrix preparation: E = exp(A) and G = E o A, zero padded ----
__global__ void pe_prepare_kernel(const float *__restrict__ A, float *__restrict__ E, float *__restrict__ G, int S) {
    const int Sp = padded_states(S), Mp = padded_rows(S);
    const size_t n = (size_t)Mp * Sp;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(e / Sp), k = (int)(e % Sp);
        float x = 0.f, g = 0.f;
        if (r < S && k < S) {
            const float a = A[(size_t)r * S + k];
            x = expf(a);
            g = a == -INFINITY ? 0.f : x * a;
        }
        E[e] = x;
        G[e] = g;
    }
}

// ---- first frame: a_0 = exp(pi + o_0 - m_0), h_0 = 0; grid (B, ceil(S / 256)) ----
__global__ void pe_first_kernel(const float *__restrict__ obs, const float *__restrict__ initial, const float *__restrict__ m,
                                float *__restrict__ a_out, float *__restrict__ h_out, float *__restrict__ partial, int T, int S) {
    const int b = blockIdx.x, j = blockIdx.y * blockDim.x + threadIdx.x;
    const size_t row = (size_t)b * T;
    const int Sp = padded_states(S);
    float v = 0.f;
    if (j < S) v = expf(initial[j] + obs[row * S + j] - m[row]);
    const float s = sum32(v);
    if (j < S) {
        a_out[(size_t)b * Sp + j] = v;
        h_out[(size_t)b * Sp + j] = 0.f;
    }
    if ((threadIdx.x & 31) == 0 && j < S) partial[(size_t)b * partials_of(S) + j / fb::kRowsPerPartial] = s;
}

// ---- one frame t >= 1: d = E p, D2 = E u, D3 = G p over a 32 x 32 tile of (states, items) ----
//
// The operand layout, the K split over the KS waves of the workgroup and the two forms are fb_step_kernel's: lane l holds
// row l & 31 of both matrices and column l & 31 of both operands, k = 8 chunk + 4 (l >> 5) + r in MFMA r of a chunk.
//   STAGED (many tiles): KS = 4, the workgroup stages 64-wide K blocks of E, G, p and u in LDS, the next block's loads in
//       flight in registers while this one is multiplied; wave w takes chunks w and w + 4 of every block.
//   direct (few tiles): KS = 1, 2 or 4 waves read their interleaved chunks straight from global memory.
// p_in, u_in: rows of frame t - 1 ([B][Sp], every float4 of a row readable: the item kernel zeroes columns >= S);
// a_out, h_out, partial: rows of frame t.  Items with t >= F write nothing.
template <bool STAGED>
__global__ __launch_bounds__(256) void pe_step_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                      const float *__restrict__ E, const float *__restrict__ G,
                                                      const float *__restrict__ m, const float *__restrict__ p_in,
                                                      const float *__restrict__ u_in, float *__restrict__ a_out,
                                                      float *__restrict__ h_out, float *__restrict__ partial, int t, int B,
                                                      int T, int S, int KS) {
    constexpr int TM = kStateTile, TN = kItemTile;
    // STAGED: [E, G, p, u][row][k] blocks during the products; then, like the direct form, [wave][product][col][row ^ col]
    __shared__ float smem[kStepLds];
    __shared__ int live[TN];
    const int Sp = padded_states(S), P = partials_of(S);
    const int ks = threadIdx.x / 64, lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;

    for (int q = threadIdx.x; q < TN; q += blockDim.x) {
        const int n = n0 + q;
        live[q] = (n < B && t < frames_of(frames, n, T)) ? 1 : 0;
    }
    auto item_row = [&](int n) { return (size_t)(n < B ? n : B - 1) * Sp; };     // (columns beyond B are computed and dropped)

    f32x16 acc_d = {}, acc_2 = {}, acc_3 = {};
    if constexpr (STAGED) {
        // thread: row tid / 8 of all four blocks, k = 4 (tid % 8) + 32 i of the block: each load instruction covers whole lines
        const int lrow = threadIdx.x >> 3, lk = 4 * (threadIdx.x & 7);
        const float *gE = E + (size_t)(m0 + lrow) * Sp + lk;
        const float *gG = G + (size_t)(m0 + lrow) * Sp + lk;
        const float *gP = p_in + item_row(n0 + lrow) + lk;
        const float *gU = u_in + item_row(n0 + lrow) + lk;
        const int blocks = (S + kBlockK - 1) / kBlockK;
        constexpr int LI = kBlockK / 32;
        f32x4 re[LI], rg[LI], rp[LI], ru[LI];
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        auto fetch = [&](int blk) {
#pragma unroll
            for (int i = 0; i < LI; ++i) {
                const int off = blk * kBlockK + 32 * i;
                const bool in = off + lk < Sp;
                re[i] = in ? *reinterpret_cast<const f32x4 *>(gE + off) : zero;
                rg[i] = in ? *reinterpret_cast<const f32x4 *>(gG + off) : zero;
                rp[i] = in ? *reinterpret_cast<const f32x4 *>(gP + off) : zero;
                ru[i] = in ? *reinterpret_cast<const f32x4 *>(gU + off) : zero;
            }
        };
        float *const sE = smem, *const sG = smem + 32 * kLdsStride, *const sP = smem + 64 * kLdsStride,
                     *const sU = smem + 96 * kLdsStride;
        fetch(0);
        for (int blk = 0; blk < blocks; ++blk) {
            if (blk > 0) __syncthreads();                           // every wave is done with the previous block
#pragma unroll
            for (int i = 0; i < LI; ++i) {
                const int at = lrow * kLdsStride + 32 * i + lk;
                *reinterpret_cast<f32x4 *>(sE + at) = re[i];
                *reinterpret_cast<f32x4 *>(sG + at) = rg[i];
                *reinterpret_cast<f32x4 *>(sP + at) = rp[i];
                *reinterpret_cast<f32x4 *>(sU + at) = ru[i];
            }
            __syncthreads();
            if (blk + 1 < blocks) fetch(blk + 1);                   // the next block's loads fly during this block's MFMAs
#pragma unroll
            for (int c = ks; c < kBlockK / 8; c += 4) {
                if (blk * kBlockK + 8 * c >= S) break;
                const int at = l32 * kLdsStride + 8 * c + 4 * h;
                const f32x4 e = *reinterpret_cast<const f32x4 *>(sE + at);
                const f32x4 g = *reinterpret_cast<const f32x4 *>(sG + at);
                const f32x4 xp = *reinterpret_cast<const f32x4 *>(sP + at);
                const f32x4 xu = *reinterpret_cast<const f32x4 *>(sU + at);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    acc_d = __builtin_amdgcn_mfma_f32_32x32x2f32(e[r], xp[r], acc_d, 0, 0, 0);
                    acc_2 = __builtin_amdgcn_mfma_f32_32x32x2f32(e[r], xu[r], acc_2, 0, 0, 0);
                    acc_3 = __builtin_amdgcn_mfma_f32_32x32x2f32(g[r], xp[r], acc_3, 0, 0, 0);
                }
            }
        }
        __syncthreads();                                            // (the reduction below reuses the staging LDS)
    } else {
        const float *erow = E + (size_t)(m0 + l32) * Sp;           // < Mp: padded rows are zero
        const float *grow = G + (size_t)(m0 + l32) * Sp;
        const float *prow = p_in + item_row(n0 + l32);
        const float *urow = u_in + item_row(n0 + l32);
        const int chunks = (S + 7) / 8;                             // 8 chunks <= Sp
        for (int kc = ks; kc < chunks; kc += KS) {
            const int k = 8 * kc + 4 * h;
            const f32x4 e = *reinterpret_cast<const f32x4 *>(erow + k);
            const f32x4 g = *reinterpret_cast<const f32x4 *>(grow + k);
            const f32x4 xp = *reinterpret_cast<const f32x4 *>(prow + k);
            const f32x4 xu = *reinterpret_cast<const f32x4 *>(urow + k);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc_d = __builtin_amdgcn_mfma_f32_32x32x2f32(e[r], xp[r], acc_d, 0, 0, 0);
                acc_2 = __builtin_amdgcn_mfma_f32_32x32x2f32(e[r], xu[r], acc_2, 0, 0, 0);
                acc_3 = __builtin_amdgcn_mfma_f32_32x32x2f32(g[r], xp[r], acc_3, 0, 0, 0);
            }
        }
    }
    // D layout: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float *mine = smem + (size_t)ks * 3 * 1024;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int r = (reg & 3) + 8 * (reg >> 2) + 4 * h;
        const int at = l32 * 32 + (r ^ l32);
        mine[at] = acc_d[reg];
        mine[1024 + at] = acc_2[reg];
        mine[2048 + at] = acc_3[reg];
    }
    __syncthreads();

    // epilogue: consecutive threads take consecutive rows of one item; the waves' tiles are summed in wave order
    for (int idx = threadIdx.x; idx < TM * TN; idx += blockDim.x) {
        const int jl = idx % TM, nl = idx / TM;
        const int j = m0 + jl, item = n0 + nl;
        const int at = nl * 32 + (jl ^ nl);
        float d = 0.f, d2 = 0.f, d3 = 0.f;
        for (int q = 0; q < KS; ++q) {
            const float *tile = smem + (size_t)q * 3 * 1024 + at;
            d += tile[0];
            d2 += tile[1024];
            d3 += tile[2048];
        }
        const bool on = j < S && item < B && live[nl];
        float v = 0.f, hh = 0.f;
        if (on) {
            const size_t frame = (size_t)item * T + t;
            v = expf(obs[frame * S + j] - m[frame]) * d;
            hh = d == 0.f ? 0.f : logf(d) + (d2 - d3) / d;
        }
        const float total = sum32(v);
        if (on) {
            a_out[(size_t)item * Sp + j] = v;
            h_out[(size_t)item * Sp + j] = hh;
            if (jl == 0) partial[(size_t)item * P + j / fb::kRowsPerPartial] = total;
        }
    }
}

// ---- one frame of one item: c_t from the partials in order, p_t = a_t / c_t and u_t = p_t h_t - xlogx(p_t) in place,
// prefix_t = sum_j u_t[j] in fp64 (a lane's states in order, then a fixed tree), columns [S, Sp) zeroed.  grid (B), block 256.
// Frames t >= F: prefix_t = 0, nothing else.
__global__ __launch_bounds__(256) void pe_item_kernel(const int32_t *__restrict__ frames, const float *__restrict__ partial,
                                                      float *__restrict__ p, float *__restrict__ u, float *__restrict__ cbuf,
                                                      float *__restrict__ prefix, int t, int T, int S) {
    __shared__ double part[256];
    __shared__ float csum;
    const int b = blockIdx.x, Sp = padded_states(S);
    const size_t frame = (size_t)b * T + t;
    if (t >= frames_of(frames, b, T)) {
        if (threadIdx.x == 0) prefix[frame] = 0.f;
        return;
    }
    if (threadIdx.x == 0) csum = fb::row_sum(partial, (size_t)b, partials_of(S));
    __syncthreads();
    const float c = csum;
    float *const prow = p + (size_t)b * Sp, *const urow = u + (size_t)b * Sp;
    double acc = 0.;
    for (int j = threadIdx.x; j < Sp; j += 256) {
        float pj = 0.f, uj = 0.f;
        if (j < S) {
            const float a = prow[j];
            pj = c == 0.f ? a * 0.f : a / c;                        // (a frame of zero probability: 0, or NaN from NaN)
            uj = pj * urow[j] - xlogx(pj);
            acc += (double)uj;
        }
        prow[j] = pj;
        urow[j] = uj;
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
        if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        prefix[frame] = (float)part[0];
        cbuf[frame] = c;
    }
}

// ---- L = sum (log c_t + m_t) in fp64, H = prefix_{F-1}; an item whose L is not finite gets a NaN entropy and NaN in its
// prefix entries t < F (L itself stays -inf for an item of total probability 0).  One workgroup per item.
__global__ __launch_bounds__(256) void pe_final_kernel(const int32_t *__restrict__ frames, const float *__restrict__ m,
                                                       const float *__restrict__ cbuf, float *__restrict__ prefix,
                                                       float *__restrict__ entropy, float *__restrict__ loglik, int T) {
    __shared__ double part[256];
    const int b = blockIdx.x, F = frames_of(frames, b, T);
    double acc = 0.;
    for (int t = threadIdx.x; t < F; t += blockDim.x) {
        const size_t row = (size_t)b * T + t;
        acc += log((double)cbuf[row]) + (double)m[row];
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
        if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
        __syncthreads();
    }
    const double L = part[0];
    const bool bad = L != L || L == INFINITY || L == -INFINITY;
    if (threadIdx.x == 0) {
        loglik[b] = (L != L || L == INFINITY) ? NAN : (float)L;
        entropy[b] = bad ? NAN : prefix[(size_t)b * T + F - 1];
    }
    if (!bad) return;
    for (int t = threadIdx.x; t < F; t += blockDim.x) prefix[(size_t)b * T + t] = NAN;
}

// ---- uniform transition: frames are independent.  One wave per (item, frame): the entropy of softmax(x) and its
// log-sum-exp, x = o_t (t = 0: pi + o_0).  With z = x - max x, s = sum exp z and w = sum z exp z (0 where exp z = 0):
// rowh = log s - w / s, lse = max x + log s, both in fp64 from the fp32 sums.  Rows t >= F are not written.
template <bool VEC>
__global__ __launch_bounds__(256) void pe_uniform_rows_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                              const float *__restrict__ initial, double *__restrict__ rowh,
                                                              double *__restrict__ lse, int B, int T, int S) {
    const size_t rowi = (size_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (rowi >= (size_t)B * T) return;
    const int b = (int)(rowi / T), t = (int)(rowi % T);
    if (t >= frames_of(frames, b, T)) return;
    const float *o = obs + rowi * S;
    const bool first = t == 0;
    float mu, s = 0.f, w = 0.f;
    if (VEC && !first && S <= 4 * 64 * kRowRegs) {
        // the row in registers: one read of the observation
        f32x4 v[kRowRegs];
        float mx = -INFINITY;
#pragma unroll
        for (int q = 0; q < kRowRegs; ++q) {
            const int j = 4 * (lane + 64 * q);
            v[q] = j < S ? *reinterpret_cast<const f32x4 *>(o + j) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            mx = nan_max(nan_max(mx, v[q][0]), nan_max(nan_max(v[q][1], v[q][2]), v[q][3]));
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = nan_max(mx, __shfl_xor(mx, off, 64));
        mu = mx == -INFINITY ? 0.f : mx;
#pragma unroll
        for (int q = 0; q < kRowRegs; ++q) {
            float e[4], ze[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z = v[q][r] - mu;
                e[r] = expf(z);
                ze[r] = e[r] > 0.f ? z * e[r] : 0.f;
            }
            s += (e[0] + e[1]) + (e[2] + e[3]);
            w += (ze[0] + ze[1]) + (ze[2] + ze[3]);
        }
    } else {
        // longer rows, unaligned rows and the first frame: two passes, the second from L1 / L2.  A lane takes the states
        // the register form gives it and sums them in its order, so a row's bits are the same in both forms.
        float mx = -INFINITY;
        for (int j = lane; j < S; j += 64) mx = nan_max(mx, first ? initial[j] + o[j] : o[j]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = nan_max(mx, __shfl_xor(mx, off, 64));
        mu = mx == -INFINITY ? 0.f : mx;
        for (int q = 0; 256 * q < S; ++q) {
            float e[4], ze[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 4 * (lane + 64 * q) + r;
                const float z = (j < S ? (first ? initial[j] + o[j] : o[j]) : -INFINITY) - mu;
                e[r] = expf(z);
                ze[r] = e[r] > 0.f ? z * e[r] : 0.f;
            }
            s += (e[0] + e[1]) + (e[2] + e[3]);
            w += (ze[0] + ze[1]) + (ze[2] + ze[3]);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s += __shfl_xor(s, off, 64);
        w += __shfl_xor(w, off, 64);
    }
    if (lane == 0) {
        const double ls = log((double)s);
        rowh[rowi] = ls - (double)w / (double)s;
        lse[rowi] = (double)mu + ls;
    }
}

// The running sums of an item in fp64, a lane per item: L = lse_0 + sum_{t>=1} (uniform + lse_t), prefix_t = sum_{s<=t}
// rowh_s, H = prefix_{F-1}; the non-finite rules of pe_final_kernel; prefix entries t >= F are 0.  `prefix` may be null.
__global__ __launch_bounds__(64) void pe_uniform_scan_kernel(const int32_t *__restrict__ frames, const double *__restrict__ rowh,
                                                             const double *__restrict__ lse, float uniform,
                                                             float *__restrict__ entropy, float *__restrict__ prefix,
                                                             float *__restrict__ loglik, int B, int T) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int F = frames_of(frames, b, T);
    const size_t at = (size_t)b * T;
    double L = 0., H = 0.;
    for (int t = 0; t < F; ++t) {
        L += (t == 0 ? 0. : (double)uniform) + lse[at + t];
        H += rowh[at + t];
    }
    const bool bad = L != L || L == INFINITY || L == -INFINITY;
    loglik[b] = (L != L || L == INFINITY) ? NAN : (float)L;
    entropy[b] = bad ? NAN : (float)H;
    if (!prefix) return;
    double run = 0.;
    for (int t = 0; t < T; ++t) {
        if (t < F) run += rowh[at + t];
        prefix[at + t] = t >= F ? 0.f : (bad ? NAN : (float)run);
    }
}

}  // namespace pe
