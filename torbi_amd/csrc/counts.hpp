// counts.hpp -- expected transition counts and initial-state counts of the HMM the decoder decodes
// (torbi_hip_forward_backward_counts, torbi_amd/training.py, POSTERIOR.md "Expected counts").
//
// With the scaled quantities of forward_backward.hpp (a_t unnormalised forward rows, c_t their sums, w_t the backward
// operand) and a per-item weight g_b:
//     X = E (.) sum_b g_b sum_{t=1}^{F_b-1} w_t^b (x) (a_{t-1}^b / c_{t-1}^b)      I = sum_b g_b gamma_0^b
// Pair t is consumed by one launch of fb_counts_kernel between backward step t (or the last-frame kernel, which write
// w_t) and backward step t - 1 (which turns a_{t-1} into gamma_{t-1} in place and, one step later, reuses w_t's buffer).
// Each launch is a rank-B update of the (S, S) fp32 accumulator, which is the caller's counts_out: the first launch
// (t = T - 1) stores, the later ones add, and fb_counts_finalize_kernel multiplies by E at the end.  So the sum over t runs
// from T - 1 down to 1 and the sum over items in item order inside each product: the bits depend on the inputs only.
// Items with t >= F_b, g_b == 0 or a non-finite L_b are skipped: their operand columns are selected to 0, not multiplied.
#pragma once

#include "forward_backward.hpp"

namespace fb {

constexpr int kCountsTile = 64;             // 64 x 64 outputs per workgroup, 32 x 32 per wave (2 x 2 waves)
constexpr int kCountsBlockK = 64;           // items per LDS stage
constexpr int kCountsStride = 68;           // (68: like 132 in fb_step_kernel, 16 rows of float4 reads cover all banks once)

// ---- one pair t: counts[j][i] (=|+=) sum_b W[b][j] * Ahat[b][i] over a 64 x 64 tile; grid (S / 64 on i, S / 64 on j) ----
//
// Both operands are item-major ([B][S], state contiguous), so K (the item) runs across rows.  Thread q of the workgroup
// loads states 4 (q % 16) .. +3 of items 4 (q / 16) .. +3 of a 64-item block of both operands (16 threads read one
// 256-B run of an item row), transposes the 4 x 4 in registers and writes the block to LDS as [state][item]: the MFMA
// loop then reads one float4 (4 consecutive items) per operand and lane, the k order of fb_step_kernel.  The next block's
// loads fly during this block's MFMAs.
//   W[b][j]    = w_t^b[j]                                   (the backward operand, buffer w + (t & 1) B Sp)
//   Ahat[b][i] = a_{t-1}^b[i] * (g_b / c_{t-1}^b)           (row t - 1 of `post`, still unnormalised)
template <bool VEC>
__global__ __launch_bounds__(256) void fb_counts_kernel(const int32_t *__restrict__ frames, const float *__restrict__ weights,
                                                        const float *__restrict__ loglik, const float *__restrict__ cbuf,
                                                        const float *__restrict__ post, const float *__restrict__ w,
                                                        float *__restrict__ counts, int t, int B, int T, int S, int first) {
    __shared__ float lw[kCountsTile * kCountsStride], la[kCountsTile * kCountsStride];
    const int Sp = padded_states(S);
    const int wave = threadIdx.x / 64, lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const int wj = wave >> 1, wi = wave & 1;
    const int I0 = blockIdx.x * kCountsTile, J0 = blockIdx.y * kCountsTile;
    const int sq = threadIdx.x & 15, iq = threadIdx.x >> 4;
    f32x4 rw[4], ra[4];
    auto fetch = [&](int blk) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int b = blk * kCountsBlockK + 4 * iq + q;
            f32x4 x = {0.f, 0.f, 0.f, 0.f}, y = {0.f, 0.f, 0.f, 0.f};
            if (b < B) {
                // every load of the item is issued at once (all are in bounds for b < B); the item's operands are then
                // selected, so a skipped item's stale or NaN values never reach the product
                const float g = weights ? weights[b] : 1.f;
                const int F = frames_of(frames, b, T);
                const float L = loglik[b], c = cbuf[(size_t)b * T + t - 1];
                const int j = J0 + 4 * sq, i = I0 + 4 * sq;
                if (j < S) {                                        // (j + 3 < Sp: rows of w are padded to 32)
                    x = *reinterpret_cast<const f32x4 *>(w + (size_t)b * Sp + j);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (j + r >= S) x[r] = 0.f;                 // (the padding of w is never written)
                }
                const float *arow = post + ((size_t)b * T + (t - 1)) * S;
                if (VEC) {
                    if (i < S) y = *reinterpret_cast<const f32x4 *>(arow + i);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[r] = i + r < S ? arow[i + r] : 0.f;
                }
                if (t < F && g != 0.f && isfinite(L)) {
                    y *= g / c;
                } else {
                    x = f32x4{0.f, 0.f, 0.f, 0.f};
                    y = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
            rw[q] = x;
            ra[q] = y;
        }
    };
    f32x16 acc = {};
    const int blocks = (B + kCountsBlockK - 1) / kCountsBlockK;
    fetch(0);
    for (int blk = 0; blk < blocks; ++blk) {
        if (blk > 0) __syncthreads();                               // every wave is done with the previous block
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            *reinterpret_cast<f32x4 *>(lw + (4 * sq + r) * kCountsStride + 4 * iq) = f32x4{rw[0][r], rw[1][r], rw[2][r], rw[3][r]};
            *reinterpret_cast<f32x4 *>(la + (4 * sq + r) * kCountsStride + 4 * iq) = f32x4{ra[0][r], ra[1][r], ra[2][r], ra[3][r]};
        }
        __syncthreads();
        if (blk + 1 < blocks) fetch(blk + 1);
#pragma unroll
        for (int c = 0; c < kCountsBlockK / 8; ++c) {
            if (blk * kCountsBlockK + 8 * c >= B) break;
            const int kk = 8 * c + 4 * h;
            const f32x4 a = *reinterpret_cast<const f32x4 *>(lw + (32 * wj + l32) * kCountsStride + kk);
            const f32x4 x = *reinterpret_cast<const f32x4 *>(la + (32 * wi + l32) * kCountsStride + kk);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r], x[r], acc, 0, 0, 0);
        }
    }
    // D layout: col (i) = lane & 31, row (j) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5); 32 lanes store one 128-B run
    const int i = I0 + 32 * wi + l32;
    if (i >= S) return;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int j = J0 + 32 * wj + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (j < S) {
            float *p = counts + (size_t)j * S + i;
            *p = first ? acc[reg] : *p + acc[reg];
        }
    }
}

// ---- X = E (.) accumulator, in place; with no pair at all (T = 1) the accumulator is 0 ----
__global__ void fb_counts_finalize_kernel(const float *__restrict__ E, float *__restrict__ counts, int S, int has_pairs) {
    const int Sp = padded_states(S);
    const size_t n = (size_t)S * S;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(e / S), i = (int)(e % S);
        counts[e] = E[(size_t)j * Sp + i] * (has_pairs ? counts[e] : 0.f);
    }
}

// ---- I[j] = sum_b g_b gamma_0^b[j] in item order, skipped items excluded; grid S / 256 ----
__global__ __launch_bounds__(256) void fb_initial_counts_kernel(const float *__restrict__ weights,
                                                                const float *__restrict__ loglik,
                                                                const float *__restrict__ post,
                                                                float *__restrict__ initial_counts, int B, int T, int S) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= S) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) {
        const float g = weights ? weights[b] : 1.f;
        if (g != 0.f && isfinite(loglik[b])) s += g * post[(size_t)b * T * S + j];
    }
    initial_counts[j] = s;
}

}  // namespace fb
