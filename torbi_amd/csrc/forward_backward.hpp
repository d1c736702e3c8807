// forward_backward.hpp -- per-frame state posteriors and sequence log-likelihood of the HMM the decoder decodes
// (torbi_hip_forward_backward / _uniform, torbi_amd/posterior.py, POSTERIOR.md).
//
// The sum-product recurrence in linear space with per-frame rescaling.  With E = exp(A) ([next][prev]),
// m_t = max_j o_t[j] (t = 0: max_j (pi + o_0)[j]) and e_t = exp(o_t - m_t) in [0, 1]:
//     a_0 = exp(pi + o_0 - m_0)                      c_t = sum_j a_t[j]   (fixed order: 32-row partials, then in order)
//     a_t = e_t * (E a_{t-1}) / c_{t-1}              L   = sum_{t<F} (log c_t + m_t)             (fp64)
//     w_{F-1} = e_{F-1} / c_{F-1},  b_{F-1} = 1
//     b_t = E^T w_{t+1},  w_t = e_t * b_t / c_t     gamma_t = a_t * b_t / c_t
// Each step is a GEMM with M = states, K = states and N = items on the f32 MFMA (v_mfma_f32_32x32x2_f32); the unnormalised
// rows a_t live in the caller's posterior buffer and are turned into gamma in place by the backward steps.
//
// Workspace (torbi_hip_forward_backward_workspace_bytes), every piece 256-B aligned:
//     E, Et    [Mp][Sp] fp32   exp(A) and its transpose, rows >= S and columns >= S zero (Mp = S up to 64, Sp = S up to 32)
//     m        [B][T]   fp32   row maxima (-inf replaced by 0: a row of zero probability keeps e = 0, not NaN)
//     c        [B][T]   fp32   row sums c_t (written by the log-likelihood kernel, read by the backward steps)
//     partial  [B][T][ceil(S/32)] fp32   per-32-row sums of a_t, summed in order into c_t
//     w        [2][B][Sp] fp32 backward operand, by parity of t
// The uniform route uses the first B*T*8 bytes as the per-row log-sum-exp (fp64).
//
// One launch per timestep and pass: nothing waits across workgroups, and a call captures into a graph.  Output column n of
// an MFMA reads column n of the operand only, so an item's bits never depend on other items' data.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "scratch.hpp"

namespace fb {

constexpr int kRowsPerPartial = 32;          // one partial sum per 32 rows of a_t
constexpr int kMaxWaves = 16;                // per workgroup of a step kernel (64 KB of LDS for the split-K reduction)
constexpr int kMaxStates = 16384;
constexpr int kRowRegs = 8;                 // float4 per lane of a uniform-route row held in registers (S <= 2048)

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__host__ __device__ inline int padded_states(int S) { return (int)align_up((size_t)S, 32); }
__host__ __device__ inline int padded_rows(int S) { return (int)align_up((size_t)S, 64); }
__host__ __device__ inline int partials_of(int S) { return (S + kRowsPerPartial - 1) / kRowsPerPartial; }

struct Layout {
    float *E, *Et, *m, *c, *partial, *w;
    size_t total;
};

// `base`: the caller's workspace aligned up to 256 bytes, or null for the byte count alone
inline Layout layout(char *base, int B, int T, int S) {
    const size_t Sp = (size_t)padded_states(S), Mp = (size_t)padded_rows(S), BT = (size_t)B * T;
    Scratch a(base);
    Layout l;
    l.E = a.take<float>(Mp * Sp);
    l.Et = a.take<float>(Mp * Sp);
    l.m = a.take<float>(BT);
    l.c = a.take<float>(BT);
    l.partial = a.take<float>(BT * (size_t)partials_of(S));
    l.w = a.take<float>((size_t)2 * B * Sp);
    l.total = a.bytes + 256;                 // (room to align the caller's base)
    return l;
}

__device__ __forceinline__ int frames_of(const int32_t *frames, int b, int T) {
    const int f = frames[b];
    return f < 1 ? 1 : (f > T ? T : f);
}

// max that returns NaN when either operand is NaN (fmaxf drops it)
__device__ __forceinline__ float nan_max(float a, float b) {
    float r = fmaxf(a, b);
    if (a != a) r = a;
    if (b != b) r = b;
    return r;
}

// sum of 32 consecutive lanes (lanes 0-31 and 32-63 of a wave separately), every lane gets its group's sum; fixed order
__device__ __forceinline__ float sum32(float x) {
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// c_t of item b: its partial sums in order
__device__ __forceinline__ float row_sum(const float *partial, size_t row, int P) {
    const float *p = partial + row * P;
    float s = 0.f;
#pragma unroll 8
    for (int q = 0; q < P; ++q) s += p[q];
    return s;
}

// ---- matrix preparation: E = exp(A) and E^T, zero padded ----
__global__ void fb_prepare_kernel(const float *__restrict__ A, float *__restrict__ E, float *__restrict__ Et, int S) {
    const int Sp = padded_states(S), Mp = padded_rows(S);
    const size_t n = (size_t)Mp * Sp;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(e / Sp), k = (int)(e % Sp);
        E[e] = (r < S && k < S) ? expf(A[(size_t)r * S + k]) : 0.f;
        Et[e] = (r < S && k < S) ? expf(A[(size_t)k * S + r]) : 0.f;
    }
}

// ---- row maxima: one wave per (item, frame); frames an item does not have are not read ----
__global__ void fb_rowmax_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                 const float *__restrict__ initial, float *__restrict__ m, int B, int T, int S) {
    const size_t row = (size_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (row >= (size_t)B * T) return;
    const int b = (int)(row / T), t = (int)(row % T);
    if (t >= frames_of(frames, b, T)) {
        if (lane == 0) m[row] = 0.f;
        return;
    }
    const float *o = obs + row * S;
    float x = -INFINITY;
    for (int j = lane; j < S; j += 64) x = nan_max(x, t == 0 ? initial[j] + o[j] : o[j]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = nan_max(x, __shfl_xor(x, off, 64));
    if (lane == 0) m[row] = x == -INFINITY ? 0.f : x;
}

// ---- first frame: a_0 = exp(pi + o_0 - m_0); grid (B, ceil(S / 256)) ----
__global__ void fb_forward_first_kernel(const float *__restrict__ obs, const float *__restrict__ initial,
                                        const float *__restrict__ m, float *__restrict__ post, float *__restrict__ partial,
                                        int T, int S) {
    const int b = blockIdx.x, j = blockIdx.y * blockDim.x + threadIdx.x;
    const size_t row = (size_t)b * T;
    float v = 0.f;
    if (j < S) v = expf(initial[j] + obs[row * S + j] - m[row]);
    const float s = sum32(v);
    if (j < S) post[row * S + j] = v;
    if ((threadIdx.x & 31) == 0 && j < S) partial[row * partials_of(S) + j / kRowsPerPartial] = s;
}

// ---- one step of either pass: D[j][n] = sum_k Mat[j][k] * X[n][k] over a 32 x 32 tile of (states, items) ----
//
// Lane l of a wave holds row l & 31 of the matrix and column l & 31 of the operand, k = 8 chunk + 4 (l >> 5) + r in MFMA r
// of an 8-wide chunk (the same k order on both operands, so one float4 per operand and chunk).  K is split over the KS
// waves of the workgroup; their partial tiles meet in LDS, summed in wave order.
//   STAGED (many tiles): KS = 4.  The workgroup stages 128-wide K blocks of both operands in LDS (each global load
//       instruction reads whole 128-B lines; the next block is loaded into registers while this one is multiplied) and
//       wave w takes chunks w, w + 4, ... of every block.
//   direct (few tiles, e.g. one item): KS = 1 .. 16 waves read their interleaved chunks straight from global memory.
//
// BACKWARD = false (frame t >= 1): X = a_{t-1} rows in `post` (stride S), a_t[j] = e_t[j] * D / c_{t-1} written to row t
//     of `post` with its 32-row partial sums; rows t >= F are zero.
// BACKWARD = true (frame t <= T - 2): X = w_{t+1} (stride Sp), items with t < F - 1 only: b_t = D,
//     gamma_t = a_t * b_t / c_t in place (NaN where L is not finite), w_t = e_t * b_t / c_t.
constexpr int kBlockK = 128, kLdsStride = 132;  // (132: the float4 operand reads of 16 rows cover all 64 banks once)
template <bool STAGED, bool BACKWARD, bool VEC>
__global__ __launch_bounds__(1024) void fb_step_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                       const float *__restrict__ mat, const float *__restrict__ m,
                                                       const float *__restrict__ cbuf, float *__restrict__ partial,
                                                       const float *__restrict__ loglik, float *__restrict__ post,
                                                       const float *__restrict__ x_in, float *__restrict__ w_out, int t, int B,
                                                       int T, int S, int KS) {
    constexpr int TM = 32, TN = 32, SUB = 1;
    // STAGED: [matrix, operand][row][k] blocks during the product; then, like the direct form, [wave][col][row ^ col]
    __shared__ float smem[STAGED ? 2 * 32 * kLdsStride : kMaxWaves * 1024];
    float *const red = smem;
    __shared__ float scale[TN];                      // c (forward: c_{t-1}; backward: c_t) per item of the tile
    __shared__ int live[TN];
    const int Sp = padded_states(S), P = partials_of(S);
    const int wave = threadIdx.x / 64, lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const int sub = 0, ks = wave;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;

    // per item of the tile: does it take part in this step, and its c
    for (int q = threadIdx.x; q < TN; q += blockDim.x) {
        const int n = n0 + q;
        int on = 0;
        float c = 1.f;
        if (n < B) {
            const int F = frames_of(frames, n, T);
            if (!BACKWARD) {
                on = t < F ? 1 : 0;
                if (on) c = row_sum(partial, (size_t)n * T + t - 1, P);
            } else {
                on = t < F - 1 ? 1 : 0;
                if (on) c = cbuf[(size_t)n * T + t];
            }
        }
        live[q] = on;
        scale[q] = c;
    }

    const size_t xstride = BACKWARD ? (size_t)Sp : (size_t)S;
    auto operand_row = [&](int n) {
        n = n < B ? n : B - 1;                                      // (columns beyond B are computed and dropped)
        return BACKWARD ? x_in + (size_t)n * xstride : x_in + ((size_t)n * T + (t - 1)) * xstride;
    };
    auto load_x = [&](const float *xrow, int k) {
        f32x4 x;
        if (VEC && k + 4 <= S) {
            x = *reinterpret_cast<const f32x4 *>(xrow + k);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = k + r < S ? xrow[k + r] : 0.f;
        }
        return x;
    };
    f32x16 acc = {};
    if constexpr (STAGED) {
        // thread: row tid / 8 of both blocks, k = 4 (tid % 8) + 32 i of the block: each load instruction covers whole lines
        const int lrow = threadIdx.x >> 3, lk = 4 * (threadIdx.x & 7);
        const float *gA = mat + (size_t)(m0 + lrow) * Sp + lk;
        const float *gX = operand_row(n0 + lrow);
        const int blocks = (S + kBlockK - 1) / kBlockK;
        f32x4 ra[kBlockK / 32], rx[kBlockK / 32];
        auto fetch = [&](int blk) {
#pragma unroll
            for (int i = 0; i < kBlockK / 32; ++i) {
                const int k = blk * kBlockK + 32 * i + lk;
                ra[i] = k < Sp ? *reinterpret_cast<const f32x4 *>(gA + blk * kBlockK + 32 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
                rx[i] = load_x(gX, k);
            }
        };
        fetch(0);
        for (int blk = 0; blk < blocks; ++blk) {
            if (blk > 0) __syncthreads();                           // every wave is done with the previous block
#pragma unroll
            for (int i = 0; i < kBlockK / 32; ++i) {
                *reinterpret_cast<f32x4 *>(smem + lrow * kLdsStride + 32 * i + lk) = ra[i];
                *reinterpret_cast<f32x4 *>(smem + (32 + lrow) * kLdsStride + 32 * i + lk) = rx[i];
            }
            __syncthreads();
            if (blk + 1 < blocks) fetch(blk + 1);                   // the next block's loads fly during this block's MFMAs
#pragma unroll
            for (int c = ks; c < kBlockK / 8; c += 4) {
                if (blk * kBlockK + 8 * c >= S) break;
                const int kk = 8 * c + 4 * h;
                const f32x4 a = *reinterpret_cast<const f32x4 *>(smem + l32 * kLdsStride + kk);
                const f32x4 x = *reinterpret_cast<const f32x4 *>(smem + (32 + l32) * kLdsStride + kk);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r], x[r], acc, 0, 0, 0);
            }
        }
        __syncthreads();                                            // (the reduction below reuses the staging LDS)
    } else {
        const float *arow = mat + (size_t)(m0 + l32) * Sp;         // < Mp: padded rows are zero
        const float *xrow = operand_row(n0 + l32);
        const int chunks = (S + 7) / 8;
        for (int kc = ks; kc < chunks; kc += KS) {
            const int k = 8 * kc + 4 * h;
            const f32x4 a = *reinterpret_cast<const f32x4 *>(arow + k);
            const f32x4 x = load_x(xrow, k);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r], x[r], acc, 0, 0, 0);
        }
    }
    // D layout: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float *mine = red + (size_t)(ks * SUB + sub) * 1024;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int r = (reg & 3) + 8 * (reg >> 2) + 4 * h;
        mine[l32 * 32 + (r ^ l32)] = acc[reg];
    }
    __syncthreads();

    // epilogue: consecutive threads take consecutive rows of one item
    for (int idx = threadIdx.x; idx < TM * TN; idx += blockDim.x) {
        const int jl = idx % TM, nl = idx / TM;
        const int j = m0 + jl, item = n0 + nl;
        const int s = 0, r = jl & 31, col = nl & 31;
        float d = 0.f;
        for (int q = 0; q < KS; ++q) d += red[(size_t)(q * SUB + s) * 1024 + col * 32 + (r ^ col)];
        const bool in = j < S && item < B;
        const bool on = in && live[nl];
        const size_t frame = (size_t)item * T + t;
        if (!BACKWARD) {
            float v = 0.f;
            if (on) {
                const float e = expf(obs[frame * S + j] - m[frame]);
                const float c = scale[nl];
                v = c == 0.f ? (e * d) * 0.f : (e * d) / c;         // (after a zero-probability frame: 0, or NaN from NaN)
            }
            const float total = sum32(v);
            if (in) post[frame * S + j] = v;
            if (on && r == 0) partial[frame * P + j / kRowsPerPartial] = total;
        } else if (on) {
            const float c = scale[nl];
            const float e = expf(obs[frame * S + j] - m[frame]);
            const float a = post[frame * S + j];
            const float L = loglik[item];
            post[frame * S + j] = isfinite(L) ? (a * d) / c : NAN;
            w_out[(size_t)item * Sp + j] = (e * d) / c;
        }
    }
}

// ---- log-likelihood: one workgroup per item, c_t from the partials, L = sum (log c_t + m_t) in fp64 ----
__global__ __launch_bounds__(256) void fb_loglik_kernel(const int32_t *__restrict__ frames, const float *__restrict__ m,
                                                        const float *__restrict__ partial, float *__restrict__ cbuf,
                                                        float *__restrict__ loglik, int T, int S) {
    __shared__ double part[256];
    const int b = blockIdx.x, F = frames_of(frames, b, T), P = partials_of(S);
    double acc = 0.;
    for (int t = threadIdx.x; t < F; t += blockDim.x) {
        const size_t row = (size_t)b * T + t;
        const float c = row_sum(partial, row, P);
        cbuf[row] = c;
        acc += log((double)c) + (double)m[row];
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
        if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double L = part[0];
        loglik[b] = (L != L || L == INFINITY) ? NAN : (float)L;
    }
}

// ---- last frame of each item: b = 1, gamma = a / c, w = e / c; grid (B, ceil(S / 256)) ----
__global__ void fb_backward_last_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                        const float *__restrict__ m, const float *__restrict__ cbuf,
                                        const float *__restrict__ loglik, float *__restrict__ post, float *__restrict__ w,
                                        int B, int T, int S) {
    const int b = blockIdx.x, j = blockIdx.y * blockDim.x + threadIdx.x;
    if (j >= S) return;
    const int F = frames_of(frames, b, T), t = F - 1;
    const size_t frame = (size_t)b * T + t;
    const float c = cbuf[frame];
    const float a = post[frame * S + j];
    post[frame * S + j] = isfinite(loglik[b]) ? a / c : NAN;
    const float e = t == 0 ? 0.f : expf(obs[frame * S + j] - m[frame]);    // (w_0 is never read)
    w[((size_t)(t & 1) * B + b) * padded_states(S) + j] = e / c;
}

// ---- uniform transition: gamma_0 = softmax(pi + o_0), gamma_t = softmax(o_t); one wave per (item, frame) ----
// lse[b][t] = m + log(sum exp(x - m)) in fp64; rows t >= F are zero
template <bool VEC>
__global__ __launch_bounds__(256) void fb_uniform_rows_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                              const float *__restrict__ initial, float *__restrict__ post,
                                                              double *__restrict__ lse, int B, int T, int S) {
    const size_t rowi = (size_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (rowi >= (size_t)B * T) return;
    const int b = (int)(rowi / T), t = (int)(rowi % T);
    float *out = post + rowi * S;
    if (t >= frames_of(frames, b, T)) {
        for (int j = lane; j < S; j += 64) out[j] = 0.f;
        return;
    }
    const float *o = obs + rowi * S;
    const bool first = t == 0;
    if (VEC && !first && S <= 4 * 64 * kRowRegs) {
        // the row in registers: one read of the observation, one write of the posterior
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
        const float mu = mx == -INFINITY ? 0.f : mx;
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < kRowRegs; ++q) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[q][r] = expf(v[q][r] - mu);
            s += (v[q][0] + v[q][1]) + (v[q][2] + v[q][3]);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
#pragma unroll
        for (int q = 0; q < kRowRegs; ++q) {
            const int j = 4 * (lane + 64 * q);
            if (j < S) *reinterpret_cast<f32x4 *>(out + j) = v[q] / s;
        }
        if (lane == 0) lse[rowi] = (double)mu + log((double)s);
        return;
    }
    // longer rows: three passes, the later two from L1 / L2
    // pass 1: NaN-propagating maximum
    float mx = -INFINITY;
    for (int j = lane; j < S; j += 64) mx = nan_max(mx, first ? initial[j] + o[j] : o[j]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = nan_max(mx, __shfl_xor(mx, off, 64));
    const float mu = mx == -INFINITY ? 0.f : mx;
    // pass 2: the sum
    float s = 0.f;
    for (int j = lane; j < S; j += 64) s += expf((first ? initial[j] + o[j] : o[j]) - mu);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    // pass 3: the row
    for (int j = lane; j < S; j += 64) out[j] = expf((first ? initial[j] + o[j] : o[j]) - mu) / s;
    if (lane == 0) lse[rowi] = (double)mu + log((double)s);
}

// L = lse_0 + sum_{t>=1} (u + lse_t) in fp64; an item whose L is not finite gets NaN rows t < F.  One workgroup per item.
__global__ __launch_bounds__(256) void fb_uniform_loglik_kernel(const int32_t *__restrict__ frames, const double *__restrict__ lse,
                                                                float uniform, float *__restrict__ post,
                                                                float *__restrict__ loglik, int T, int S) {
    __shared__ double part[256];
    __shared__ int bad;
    const int b = blockIdx.x, F = frames_of(frames, b, T);
    double acc = 0.;
    for (int t = threadIdx.x; t < F; t += blockDim.x) acc += (t == 0 ? 0. : (double)uniform) + lse[(size_t)b * T + t];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
        if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
        __syncthreads();
    }
    const double L = part[0];
    if (threadIdx.x == 0) {
        bad = (L != L || L == INFINITY || L == -INFINITY) ? 1 : 0;
        loglik[b] = (L != L || L == INFINITY) ? NAN : (float)L;
    }
    __syncthreads();
    if (!bad || !post) return;              // (path sampling passes no posterior)
    float *rows = post + (size_t)b * T * S;
    for (size_t e = threadIdx.x; e < (size_t)F * S; e += blockDim.x) rows[e] = NAN;
}

}  // namespace fb
