// counts_log_band.hpp -- expected transition counts in LOG SPACE on a band of up to 512 entries
// (torbi_hip_forward_backward_counts_log_band, torbi_amd/training.py forward_backward_counts_log_banded, POSTERIOR.md
// "Log-space band counts").
//
// The contract is counts_wide_band.hpp's, the model and the passes are forward_backward_log_band.hpp's:
//     band_counts[k][j] = sum_b g_b sum_{1 <= t < F_b} xi_t^b(j, j - reach_left + k)
//     xi_t(j, i) = 2^(A2[j,i] + LAop[t-1][i] + Wop[t][j])          A2 = A log2(e), fp64, rounded once
// with the operand rows fb_log_band_kernel<G, true> leaves in the workspace (`Operands` there has the identity).  The wide
// route's two factors a_{t-1}[i] g / c and w_t[j] are what leaves float32's range on a left-to-right matrix -- a[i] underflows
// while w[j] overflows, though their product is at most 1 -- so this sum cannot go to the matrix pipe: it keeps the whole
// exponent together and spends one exponential per band entry and row.  Every exponent is at most about 0.
//
// A workgroup of 256 threads owns 64 next states j (lane <-> j), a chunk of 4 DQ diagonals (wave <-> DQ of them, DQ <= 32 an
// instance) and one of KS contiguous shares of the K rows r = b T + t.  A thread keeps its DQ entries of A2, read from
// `transition` itself once, and DQ float32 sums in registers for the whole share.  K rows go through LDS in blocks of 16: of
// each row the 64 Wop values of the block and the LAop window of 64 + 4 DQ + 4 floats that starts at the chunk's first column
// rounded down to 4, loaded as 16-byte pieces, 16 threads to a row (256-byte runs); positions outside [0, S) hold -inf, and
// 2^-inf = 0 is what a clipped position adds.  The next block's pieces are in flight during this block's exponentials.  Per
// term: one LDS read (lane l reads float l + c of the window: consecutive addresses), two adds, one v_exp_f32, one fma with g_b.
//
// A row is used iff 1 <= t < F_b, g_b != 0 and L_b is finite; one that is not is never loaded and is stepped over.
//
// DQ: the band in ceil(W / 128) chunks, a quarter of a chunk up to one of 4, 8, 16, 24, 32.  KS follows the wide route's rule
// (about 1024 workgroups, at most 64 shares): a function of (B, T, S, band) alone.  Grid order: chunk fastest, then j block,
// then share.  Share s stores partial[s][j][k]; fb_log_counts_finalize_kernel adds the shares in ascending order and writes
// band_counts[k][j], 0 where the matrix clips the diagonal, NaN everywhere where the promise is broken.  The order of every
// sum is fixed by the shape: K rows ascending inside a share, shares ascending.  No float atomics, vector stores only, nothing
// waits across workgroups.
#pragma once

#include "forward_backward_log_band.hpp"

namespace fblc {

using fbl::Layout;
using fbl::Plan;
using fbl::barrier;
using fbl::f4;

constexpr int kThreads = 256;                // 4 waves
constexpr int kStates = 64;                  // next states of a workgroup
constexpr int kBlockRows = 16;               // K rows per LDS stage
constexpr int kMaxDiagonals = 32;            // of a thread
constexpr int kWorkgroups = 1024;            // what a call aims for (a constant: the workspace needs no device)
constexpr int kMaxShares = 64;

// 16-byte pieces of a row in LDS: 16 of Wop, then the window (64 + 4 DQ - 1 columns, up to 3 more in front for the rounding)
constexpr int pieces(int DQ) { return 16 + 17 + DQ; }

struct CountsPlan {
    int jblocks, chunks, dq;                 // 64-state blocks of next states; chunks of 4 dq diagonals
    int shares, per;                         // KS; K blocks of a share (the last share may hold fewer)
    long long rows;                          // B T
};
__host__ __device__ inline CountsPlan counts_plan(int B, int T, int S, const Plan &p) {
    CountsPlan c;
    c.jblocks = (S + kStates - 1) / kStates;
    const int even = (p.W + 4 * kMaxDiagonals - 1) / (4 * kMaxDiagonals);           // chunks at the widest instance
    const int quarter = ((p.W + even - 1) / even + 3) / 4;
    c.dq = quarter <= 4 ? 4 : (quarter + 7) / 8 * 8;
    c.chunks = (p.W + 4 * c.dq - 1) / (4 * c.dq);
    c.rows = (long long)B * T;
    const long long blocks = (c.rows + kBlockRows - 1) / kBlockRows;
    long long want = (kWorkgroups + c.jblocks * c.chunks - 1) / (c.jblocks * c.chunks);
    want = want > kMaxShares ? kMaxShares : want;
    want = want > blocks ? blocks : want;
    want = want < 1 ? 1 : want;
    c.per = (int)((blocks + want - 1) / want);
    c.shares = (int)((blocks + c.per - 1) / c.per);
    return c;
}

struct CountsLayout : Layout {
    float *LAop, *Wop;                       // [B][T][S4] each
    float *Mrow;                             // [B][T]
    float *partial;                          // [KS][S][W]
    CountsPlan counts;
};

// the log route's workspace, then the operand rows, the row maxima and the planes
inline CountsLayout counts_layout(char *base, int B, int T, int S, int reach_left, int reach_right) {
    CountsLayout l;
    static_cast<Layout &>(l) = fbl::layout(base, S, reach_left, reach_right);
    l.counts = fblc::counts_plan(B, T, S, l);    // (qualified: the plan's own namespace has a counts_plan too)
    Scratch a(base, l.total - 256);
    l.LAop = a.take<float>((size_t)B * T * l.S4);
    l.Wop = a.take<float>((size_t)B * T * l.S4);
    l.Mrow = a.take<float>((size_t)B * T);
    l.partial = a.take<float>((size_t)l.counts.shares * S * l.W);
    l.total = a.bytes + 256;
    return l;
}

// a 16-byte piece of an operand row at state x (a multiple of 4, 0 <= x < S): the row's padding past S is never written
__device__ __forceinline__ f4 piece_at(const float *__restrict__ row, int x, int S) {
    f4 v = *reinterpret_cast<const f4 *>(row + x);
    if (x + 1 >= S) v.y = -INFINITY;
    if (x + 2 >= S) v.z = -INFINITY;
    if (x + 3 >= S) v.w = -INFINITY;
    return v;
}

// ---- one share of one (j block, chunk): grid jblocks * chunks * KS ----
template <int DQ>
__global__ __launch_bounds__(kThreads) void fb_log_counts_kernel(const int32_t *__restrict__ frames,
                                                                 const float *__restrict__ weights,
                                                                 const float *__restrict__ loglik, const float *__restrict__ A,
                                                                 const float *__restrict__ LAop, const float *__restrict__ Wop,
                                                                 float *__restrict__ partial, CountsPlan c, int reach_left, int W,
                                                                 int S4, int T, int S) {
    constexpr int kPieces = pieces(DQ), kStride = 4 * kPieces, kMine = (kPieces + 15) / 16;
    __shared__ __attribute__((aligned(16))) float stage[kBlockRows * kStride];      // [row][Wop 64 | window]
    __shared__ float gs[kBlockRows];                                                // g_b of a row, 0: not used
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int per_share = c.jblocks * c.chunks;
    const int share = (int)blockIdx.x / per_share, rest = (int)blockIdx.x - share * per_share;
    const int jb = rest / c.chunks, chunk = rest - jb * c.chunks;
    const int J0 = jb * kStates, k0 = chunk * 4 * DQ;                    // first next state, first diagonal
    const int first = J0 - reach_left + k0, I0 = first & ~3;             // first column; the window's (& ~3 rounds a negative one down too)
    const int j = J0 + lane, kw = k0 + DQ * wave;                        // the thread's state and first diagonal

    float a2[DQ], acc[DQ];
#pragma unroll
    for (int d = 0; d < DQ; ++d) {
        const int k = kw + d, i = j - reach_left + k;
        const bool in = k < W && j < S && i >= 0 && i < S;
        a2[d] = in ? (float)((double)A[(size_t)j * S + i] * fbl::kLog2eD) : -INFINITY;
        acc[d] = 0.f;
    }

    const int row = tid >> 4, sq = tid & 15;                             // the thread's row of a block, its first piece
    const long long blocks = (c.rows + kBlockRows - 1) / kBlockRows;
    const int blk_lo = share * c.per;
    const int blk_hi = (long long)blk_lo + c.per < blocks ? blk_lo + c.per : (int)blocks;

    f4 reg[kMine];
    float g_row;
    auto fetch = [&](int blk) __attribute__((always_inline)) {
        const long long r = (long long)blk * kBlockRows + row;
        const int b = (int)(r / T), t = (int)(r - (long long)b * T);
        g_row = 0.f;
        if (r < c.rows && t >= 1) {
            const float g = weights ? weights[b] : 1.f;
            if (t < fb::frames_of(frames, b, T) && isfinite(loglik[b])) g_row = g;
        }
#pragma unroll
        for (int m = 0; m < kMine; ++m) {
            reg[m] = f4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            const int pc = sq + 16 * m;
            if (g_row == 0.f || pc >= kPieces) continue;
            const int x = pc < 16 ? J0 + 4 * pc : I0 + 4 * (pc - 16);
            if (x < 0 || x >= S) continue;
            reg[m] = piece_at(pc < 16 ? Wop + (size_t)r * S4 : LAop + (size_t)(r - 1) * S4, x, S);
        }
    };

    fetch(blk_lo);
    const float *const mine = stage + lane, *const win = stage + kStates + (first - I0) + DQ * wave + lane;
    for (int blk = blk_lo; blk < blk_hi; ++blk) {
        if (blk > blk_lo) barrier();                                     // every wave is done with the previous block
#pragma unroll
        for (int m = 0; m < kMine; ++m)
            if (sq + 16 * m < kPieces) *reinterpret_cast<f4 *>(stage + row * kStride + 4 * (sq + 16 * m)) = reg[m];
        if (sq == 0) gs[row] = g_row;
        barrier();
        if (blk + 1 < blk_hi) fetch(blk + 1);
#pragma unroll 1
        for (int r = 0; r < kBlockRows; ++r) {                           // (a row's DQ terms are independent: enough in flight)
            const float g = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(gs[r])));
            if (g == 0.f) continue;
            const float w = mine[r * kStride];
            const float *la = win + r * kStride;
#pragma unroll
            for (int d = 0; d < DQ; ++d) acc[d] = __builtin_fmaf(g, fbl::ex2((la[d] + w) + a2[d]), acc[d]);
        }
    }

    if (j < S) {
        float *const out = partial + ((size_t)share * S + j) * W;
#pragma unroll
        for (int d = 0; d < DQ; ++d) {
            const int k = kw + d, i = j - reach_left + k;
            if (k < W && i >= 0 && i < S) out[k] = acc[d];
        }
    }
}

// ---- band_counts[k][j] = sum_s partial[s][j][k]; 0 where the matrix clips the diagonal, NaN everywhere (the initial counts
// too) where the promise is broken: fb_wide_counts_finalize_kernel's contract without the factor ----
__global__ __launch_bounds__(256) void fb_log_counts_finalize_kernel(const float *__restrict__ partial,
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
        if (i >= 0 && i < S)
            for (int q = 0; q < shares; ++q) v += partial[(size_t)q * n + e];
        band_counts[(size_t)k * S + j] = broken ? NAN : v;
    }
}

}  // namespace fblc
