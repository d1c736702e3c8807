// counts_wide_band.hpp -- expected transition counts on a band of up to 512 entries (torbi_hip_forward_backward_counts_wide_band,
// torbi_amd/training.py forward_backward_counts_wide_banded, POSTERIOR.md "Wide band counts").
//
// The contract is counts.hpp's, the model and the passes are forward_backward_wide_band.hpp's:
//     X[j, i] = E[j, i] * sum_b sum_{t=1}^{F_b-1} w_t^b[j] * (g_b a_{t-1}^b[i] / c_{t-1}^b)      j - reach_left <= i <= j + reach_right
// counts_band.hpp keeps the sum in one LDS plane [W][S] per workgroup; a plane of 175 x 1440 is 1 MB, so this route splits
// the work the other way.  fb_wide_band_operands_kernel<G> (the posterior kernel with one more arm) leaves both factors in
// the workspace, a row of S4 floats per (item, frame):
//     Wop[b][t][j] = w_t^b[j]            Aop[b][t][i] = a_t^b[i] * (g_b / c_t^b)            (rows t >= F_b are never written)
// and the sum is a GEMM whose K dimension is the (item, frame) pairs r = b T + t, of which only a band of output blocks
// exists: fb_wide_counts_kernel, on the f32 matrix pipe.
//
// A workgroup of 4 waves owns 64 next states j (a "j block"), a window of 256 prev states i that starts at the block's
// first in-band column rounded down to 4 (window chunk c: 256 c further on; 175 diagonals need one chunk, 512 need three)
// and one of KS contiguous shares of the K rows.  Wave w keeps the 64 x 64 piece of columns 64 w .. 64 w + 63 in four
// 32 x 32 accumulators of v_mfma_f32_32x32x2_f32; a wave whose columns lie outside band and matrix issues none.  K rows go
// by blocks of 64: thread q loads 4 states x 4 rows of each of the five 64-state panels (one of Wop, four of Aop), 16
// threads reading one 256-byte run of a row, transposes the 4 x 4 in registers and stores it to LDS as [state][k] with a
// stride of 68 floats (16 rows of 16-byte reads cover every bank once), the order fb_counts_kernel uses.  The next block's
// loads are in flight during this block's 128 MFMAs a wave.
//
// A row is used iff 1 <= t < F_b, g_b != 0 and L_b is finite.  One that is not is never loaded: its pieces of both panels are
// zeros, so neither the stale bytes of a row that was never written nor the NaN rows of a skipped item reach a product; the
// same holds for the states past S of a row's padding and for window columns outside the matrix.
//
// KS = min(64, K blocks, ceil(1024 / (j blocks x chunks))), then as few shares as hold the K blocks at that many blocks a
// share: a function of (B, T, S, band) alone.  Grid order: chunk fastest, then j block, then share, so the workgroups that
// read the same K rows run next to each other.  Share s stores its in-band, in-matrix cells to partial[s][j][k], k =
// i - j + reach_left (along k, so that a wave's store instruction is two 128-byte runs); fb_wide_counts_finalize_kernel adds
// the shares in order, multiplies by exp(A) and writes band_counts[k][j], 0 where the matrix clips the diagonal, NaN
// everywhere where the promise is broken.  The order of every sum is fixed by the shape: K rows ascending inside a share
// (the matrix pipe's own order within 8), shares ascending.  No float atomics, vector stores only, nothing waits across
// workgroups.
#pragma once

#include "counts.hpp"
#include "forward_backward_wide_band.hpp"

namespace fbw {

#if defined(__HIP_DEVICE_COMPILE__)
#define FBW_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define FBW_KERNEL __global__
#endif

constexpr int kCountsThreads = 256;          // 4 waves
constexpr int kCountsRows = 64;              // next states of a workgroup
constexpr int kCountsWindow = 256;           // prev states of a workgroup: 64 per wave
constexpr int kCountsBlockK = 64;            // K rows per LDS stage
constexpr int kCountsStride = kCountsBlockK + 4;
constexpr int kCountsPanels = 1 + kCountsWindow / 64;                    // 64-state panels of a stage: Wop's, then Aop's
constexpr int kCountsWorkgroups = 1024;      // what a call aims for (a constant: the workspace needs no device)
constexpr int kCountsMaxShares = 64;
constexpr size_t kCountsLdsBytes = (size_t)kCountsPanels * 64 * kCountsStride * sizeof(float);     // 87 040

typedef float f16 __attribute__((ext_vector_type(16)));   // one 32 x 32 accumulator of a lane

struct CountsPlan {
    int jblocks, chunks;                     // 64-state blocks of next states; 256-state chunks of a block's window
    int shares, per;                         // KS; K blocks of a share (the last share may hold fewer)
    long long rows;                          // B T
};
__host__ __device__ inline CountsPlan counts_plan(int B, int T, int S, const Plan &p) {
    CountsPlan c;
    c.jblocks = (S + kCountsRows - 1) / kCountsRows;
    // a block's columns run from j0 - reach_left (down to 4: up to 3 more) to j0 + 63 + reach_right: W + 66 at the most
    c.chunks = (p.W + kCountsRows + 2 + kCountsWindow - 1) / kCountsWindow;
    c.rows = (long long)B * T;
    const long long blocks = (c.rows + kCountsBlockK - 1) / kCountsBlockK;
    long long want = (kCountsWorkgroups + c.jblocks * c.chunks - 1) / (c.jblocks * c.chunks);
    want = want > kCountsMaxShares ? kCountsMaxShares : want;
    want = want > blocks ? blocks : want;
    want = want < 1 ? 1 : want;
    c.per = (int)((blocks + want - 1) / want);
    c.shares = (int)((blocks + c.per - 1) / c.per);
    return c;
}

struct CountsLayout : Layout {
    float *Wop, *Aop;                        // [B][T][S4] each
    float *partial;                          // [KS][S][W]
    CountsPlan counts;
};

// the wide route's workspace, then the operand rows and the planes
inline CountsLayout counts_layout(char *base, int B, int T, int S, int reach_left, int reach_right) {
    CountsLayout l;
    static_cast<Layout &>(l) = layout(base, B, T, S, reach_left, reach_right);
    l.counts = counts_plan(B, T, S, l);
    Scratch a(base, l.total - 256);
    l.Wop = a.take<float>((size_t)B * T * l.S4);
    l.Aop = a.take<float>((size_t)B * T * l.S4);
    l.partial = a.take<float>((size_t)l.counts.shares * S * l.W);
    l.total = a.bytes + 256;
    return l;
}

// ---- one share of one (j block, chunk): grid jblocks * chunks * KS, dynamic LDS kCountsLdsBytes ----
FBW_KERNEL __launch_bounds__(kCountsThreads) void fb_wide_counts_kernel(const int32_t *__restrict__ frames,
                                                                        const float *__restrict__ weights,
                                                                        const float *__restrict__ loglik,
                                                                        const float *__restrict__ Wop,
                                                                        const float *__restrict__ Aop,
                                                                        float *__restrict__ partial, CountsPlan c, int reach_left,
                                                                        int reach_right, int W, int S4, int B, int T, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_counts[];
    float *const lw = reinterpret_cast<float *>(lds_counts);             // [64][68]: Wop's panel
    float *const la = lw + 64 * kCountsStride;                           // [256][68]: Aop's four
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, h = lane >> 5, l32 = lane & 31;
    const int per_share = c.jblocks * c.chunks;
    const int share = (int)blockIdx.x / per_share, rest = (int)blockIdx.x - share * per_share;
    const int jb = rest / c.chunks, chunk = rest - jb * c.chunks;
    const int J0 = jb * kCountsRows;
    const int first = J0 - reach_left, I0 = (first & ~3) + chunk * kCountsWindow;       // (& ~3 rounds a negative one down too)
    // columns of the block that exist: in the band of one of its rows and in the matrix
    const int lo = first > 0 ? first : 0;
    const int last_row = J0 + kCountsRows - 1 < S - 1 ? J0 + kCountsRows - 1 : S - 1;
    const int hi = last_row + reach_right < S - 1 ? last_row + reach_right : S - 1;
    const bool active = I0 + 64 * wave <= hi && I0 + 64 * wave + 63 >= lo;            // this wave's 64 columns hold one

    const int sq = tid & 15, kq = tid >> 4;                              // the thread's quad of states in a panel, of K rows
    const long long row_end = c.rows;
    const int blk_lo = share * c.per;
    const long long blocks = (c.rows + kCountsBlockK - 1) / kCountsBlockK;
    const int blk_hi = (long long)blk_lo + c.per < blocks ? blk_lo + c.per : (int)blocks;
    // (item, frame) of the thread's first row of the share's first block; every block moves it 64 rows on
    long long r0 = (long long)blk_lo * kCountsBlockK + 4 * kq;
    int b_at = (int)(r0 / T), t_at = (int)(r0 - (long long)b_at * T);

    f4 reg[kCountsPanels][4];                                            // [panel][row of the quad]: 4 states each
    auto fetch = [&]() __attribute__((always_inline)) {
        int b = b_at, t = t_at;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int pn = 0; pn < kCountsPanels; ++pn) reg[pn][q] = f4{0.f, 0.f, 0.f, 0.f};
            bool use = r0 + q < row_end && t >= 1;
            if (use) {
                const float g = weights ? weights[b] : 1.f;
                use = t < fb::frames_of(frames, b, T) && g != 0.f && isfinite(loglik[b]);
            }
            if (use) {
                const float *wrow = Wop + (size_t)(r0 + q) * S4, *arow = Aop + (size_t)(r0 + q - 1) * S4;
                const int j = J0 + 4 * sq;
                if (j < S) {                                             // (j + 3 < S4: the rows are padded)
                    f4 x = *reinterpret_cast<const f4 *>(wrow + j);
                    if (j + 1 >= S) x.y = 0.f;                           // (the padding of a row is never written)
                    if (j + 2 >= S) x.z = 0.f;
                    if (j + 3 >= S) x.w = 0.f;
                    reg[0][q] = x;
                }
#pragma unroll
                for (int pn = 1; pn < kCountsPanels; ++pn) {
                    const int i = I0 + 64 * (pn - 1) + 4 * sq;          // (wave pn - 1's columns; nothing is loaded for a wave that idles)
                    if (i >= 0 && i < S && i - 4 * sq <= hi && i - 4 * sq + 63 >= lo) {
                        f4 y = *reinterpret_cast<const f4 *>(arow + i);
                        if (i + 1 >= S) y.y = 0.f;
                        if (i + 2 >= S) y.z = 0.f;
                        if (i + 3 >= S) y.w = 0.f;
                        reg[pn][q] = y;
                    }
                }
            }
            if (++t >= T) {                                              // the next row of the quad
                t = 0;
                ++b;
            }
        }
        r0 += kCountsBlockK;
        t_at += kCountsBlockK;
        while (t_at >= T) {
            t_at -= T;
            ++b_at;
        }
    };

    f16 acc[2][2];                                                       // [half of the 64 rows][half of the wave's 64 columns]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][x][e] = 0.f;

    fetch();
    for (int blk = blk_lo; blk < blk_hi; ++blk) {
        if (blk > blk_lo) barrier();                                     // every wave is done with the previous block
#pragma unroll
        for (int pn = 0; pn < kCountsPanels; ++pn) {
            const f4 *v = reg[pn];
            float *to = lw + (size_t)(64 * pn + 4 * sq) * kCountsStride + 4 * kq;
            *reinterpret_cast<f4 *>(to) = f4{v[0].x, v[1].x, v[2].x, v[3].x};
            *reinterpret_cast<f4 *>(to + kCountsStride) = f4{v[0].y, v[1].y, v[2].y, v[3].y};
            *reinterpret_cast<f4 *>(to + 2 * kCountsStride) = f4{v[0].z, v[1].z, v[2].z, v[3].z};
            *reinterpret_cast<f4 *>(to + 3 * kCountsStride) = f4{v[0].w, v[1].w, v[2].w, v[3].w};
        }
        barrier();
        if (blk + 1 < blk_hi) fetch();
        if (active) {
            const float *wj = lw + (size_t)l32 * kCountsStride + 4 * h;
            const float *ai = la + (size_t)(64 * wave + l32) * kCountsStride + 4 * h;
#pragma unroll
            for (int k8 = 0; k8 < kCountsBlockK; k8 += 8) {
                const f4 w0 = *reinterpret_cast<const f4 *>(wj + k8), w1 = *reinterpret_cast<const f4 *>(wj + 32 * kCountsStride + k8);
                const f4 a0 = *reinterpret_cast<const f4 *>(ai + k8), a1 = *reinterpret_cast<const f4 *>(ai + 32 * kCountsStride + k8);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[r], a0[r], acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[r], a1[r], acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[r], a0[r], acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[r], a1[r], acc[1][1], 0, 0, 0);
                }
            }
        }
    }

    // D layout: column (i) = lane & 31, row (j) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  Cell (j, i) is diagonal
    // k = i - j + reach_left of row j: 32 lanes store one run of 32 floats
    float *const plane = partial + (size_t)share * S * W;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const int i = I0 + 64 * wave + 32 * x + l32;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int j = J0 + 32 * a + (e & 3) + 8 * (e >> 2) + 4 * h, k = i - j + reach_left;
                if (j < S && i >= 0 && i < S && k >= 0 && k < W) plane[(size_t)j * W + k] = acc[a][x][e];
            }
        }
}

// ---- band_counts[k][j] = exp(A[j][i]) * sum_s partial[s][j][k], i = j - reach_left + k; 0 where the matrix clips the diagonal,
// NaN everywhere (the initial counts too) where the promise is broken: fb_band_counts_finalize_kernel's contract ----
FBW_KERNEL __launch_bounds__(256) void fb_wide_counts_finalize_kernel(const float *__restrict__ A, const float *__restrict__ partial,
                                                                      const int32_t *__restrict__ flag,
                                                                      float *__restrict__ band_counts,
                                                                      float *__restrict__ initial_counts, int shares,
                                                                      int reach_left, int W, int S) {
    const bool broken = *flag != 0;
    const size_t n = (size_t)W * S, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (broken && first < (size_t)S) initial_counts[first] = NAN;     // (the grid has at least S threads)
    for (size_t e = first; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(e / W), k = (int)(e % W);
        const int i = j - reach_left + k;
        float v = 0.f;
        if (i >= 0 && i < S) {
            float s = 0.f;
            for (int q = 0; q < shares; ++q) s += partial[(size_t)q * n + e];
            v = expf(A[(size_t)j * S + i]) * s;
        }
        band_counts[(size_t)k * S + j] = broken ? NAN : v;
    }
}

#undef FBW_KERNEL

}  // namespace fbw
