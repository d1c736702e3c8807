// forward_backward_log.hpp -- state posteriors and log-likelihood in LOG SPACE for ANY transition matrix
// (torbi_hip_forward_backward_log, torbi_amd/posterior.py forward_backward_log, POSTERIOR.md "Dense log-space route").
//
// The contract is forward_backward_log_band.hpp's with the band split taken out (natural logs, A [next][prev], F in [1, T]):
//     x_0 = pi + o_0                                   M_t = max_j x_t[j]   (-inf read as 0, NaN propagates)
//     x_t[j] = o_t[j] + lse_i (A[j,i] + la_{t-1}[i])   la_t = x_t - M_t
//     L = sum_{t<F} M_t (fp64) + lse_j la_{F-1}[j]     rounded once to fp32
//     y_{F-1} = 0    y_t[i] = lse_j (A[j,i] + r_{t+1}[j])          r_t = o_t + y_t - max_j (o_t + y_t)
//     gamma_t = softmax_j (la_t[j] + y_t[j])
// There is no promise and no flag: every float32 matrix is a valid input, -inf in it is a zero probability.
//
// Why not the matrix pipe: exp(A - blockmax) x exp(v - blockmax) on the MFMA shares one shift among a block of previous
// states.  Where the largest v of a block sits on a -inf entry of A and the next term lies 2^126 under it, the block's whole
// contribution flushes to zero -- which is what a left-to-right matrix does, and the blind spot this route exists to close.
// So every output state keeps ITS OWN running maximum (a reference of -inf read as 0), as in the band route, and the terms go
// through v_exp_f32.
//
// Inside the launches rows and packs are BASE-2 logarithms: the observation is scaled by log2(e) where it is loaded, L by
// ln 2 where it is stored.  Sp = S rounded up to the state block of 64.
//
// Launches, all on the caller's stream, nothing waits across workgroups:
//   pack   once: Pf[i][j] = A[j][i] and Pb[j][i] = A[j][i], each [Sp][Sp], (double)A * log2(e) rounded once, -inf in the
//          padding.  Both passes then read out[x] = lse_y (P[y][x] + v[y]) with lanes over x on consecutive floats.
//   step   per frame and pass, grid (ceil(B / TB) item tiles, Sp / 64 state blocks), 256 threads = 4 waves.  Lane l of every
//          wave owns output state 64 block + l; wave k walks slice k of the y range (bounds fixed by S alone).  The previous
//          rows v of the tile's TB items (la_{t-1} from `posterior` forward, r_{t+1} backward) are staged once in LDS
//          [TB][Sp] and read as 16-byte broadcasts: four v[y..y+3] of one item per ds_read_b128.  A lane loads its state's
//          entries of four pack rows (four coalesced 256-byte wave loads, the next four in flight) and reuses them from
//          registers for all TB items: matrix traffic per frame is B / TB times the pack.  Per item and four terms: four
//          adds, their maximum joins the state's running one, ONE rescaling exponential, four subtract-exp-accumulate: 1.25
//          exponentials per term, 2 TB accumulator registers.  The slices' (m, s) pairs go to LDS; one thread per (state,
//          item) combines them in slice order, adds the observation (forward: x_t into `posterior`) or not (backward: y_t
//          into the workspace).  Items with t outside their range (forward t >= F, backward t >= F - 1) are skipped, a tile
//          with none exits at once.
//   row    per frame and pass, one workgroup of 256 threads per item.  Forward: M_t (64-lane butterfly, wave values through
//          LDS: every thread holds the same bits), la_t in place, sum M_t in fp64 in the workspace, L at t = F - 1, zeros in
//          rows t >= F.  Backward: q = la + y, gamma = softmax q in place, r_t into a ping-pong buffer by the parity of t.
// The row work is not folded into the next step's staging: a step's workgroups are (state block, tile) pairs, so every
// state block would redo the row reductions of its tile (POSTERIOR.md has what the launches cost at one item).
//
// Workspace: both packs, y [B][Sp], r [2][B][Sp], sum M [B] fp64.  No (B, T, S) region: `posterior` holds x, then la, then
// gamma.  Every word that is read was written by this call first, so stale bytes do not matter.
//
// The order of every operation of an item is fixed by S alone: its bits depend neither on TB nor on its place in a tile nor
// on the batch.  No float atomics, vector stores only.
#pragma once

#include "forward_backward_log_band.hpp"

namespace fbd {

using fbl::ex2;
using fbl::f4;
using fbl::kLn2D;
using fbl::kLog2e;
using fbl::kLog2eD;
using fbl::lg2;
using fbl::ref_of;
constexpr int kThreads = 256, kWaves = 4, kSlices = 4;
constexpr int kBlockStates = 64;             // output states of a step workgroup: one per lane
constexpr int kMaxStates = fbl::kMaxStates, kMaxTile = 8;
constexpr int kMaxLdsBytes = fbl::kMaxLdsBytes;

__host__ __device__ inline int padded_states(int S) { return (S + kBlockStates - 1) / kBlockStates * kBlockStates; }
// quads of y a slice walks: the ceil(S / 4) quads in 4 equal runs (the last ones shorter or empty)
__host__ __device__ inline int slice_quads(int S) { return ((S + 3) / 4 + kSlices - 1) / kSlices; }

struct Layout { float *P[2], *y, *r; double *Msum; int Sp; size_t total; };

// `base`: the caller's workspace aligned up to 256 bytes, or null for the byte count alone
inline Layout layout(char *base, int B, int S) {
    Layout l;
    l.Sp = padded_states(S);
    Scratch a(base);
    l.P[0] = a.take<float>((size_t)l.Sp * l.Sp);
    l.P[1] = a.take<float>((size_t)l.Sp * l.Sp);
    l.y = a.take<float>((size_t)B * l.Sp);
    l.r = a.take<float>((size_t)2 * B * l.Sp);
    l.Msum = a.take<double>(B);
    l.total = a.bytes + 256;                 // (room to align the caller's base)
    return l;
}

// LDS of a step workgroup: rows [TB][Sp], slice maxima and slice sums [kSlices][TB][64] each
__host__ __device__ inline size_t lds_bytes(int TB, int S) {
    return (size_t)TB * 4 * ((size_t)padded_states(S) + 2 * kSlices * kBlockStates);
}

// ---- both packs in base 2; grid (Sp / 64, Sp / 4, 2 passes), block 256 = 4 rows y x 64 columns x ----
__global__ __launch_bounds__(256) void fb_log_dense_pack_kernel(const float *__restrict__ A, float *__restrict__ Pf,
                                                                float *__restrict__ Pb, int S, int Sp) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), pass = blockIdx.z;
    float v = -INFINITY;
    if (x < S && y < S) v = (float)((double)A[pass == 0 ? (size_t)x * S + y : (size_t)y * S + x] * kLog2eD);   // A [next][prev]
    (pass == 0 ? Pf : Pb)[(size_t)y * Sp + x] = v;
}

// ---- one step of one pass: out_b[x] = lse_y (P[y][x] + v_b[y]) (+ o_t[x] log2 e forward) for the live items of a tile ----
// forward: v_b = post[b][t - 1] (la_{t-1}), out = post[b][t];  backward: v_b = vin[b] (r_{t+1}, rows of Sp), out = yout[b]
template <int TB, bool BACKWARD>
__global__ __launch_bounds__(kThreads) void fb_log_dense_step_kernel(const float *__restrict__ obs,
                                                                     const int32_t *__restrict__ frames,
                                                                     const float *__restrict__ P, const float *__restrict__ vin,
                                                                     float *__restrict__ post, float *__restrict__ yout, int t,
                                                                     int B, int T, int S, int Sp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float *const rows = reinterpret_cast<float *>(lds_raw);              // [TB][Sp]
    float *const smax = rows + (size_t)TB * Sp;                          // [kSlices][TB][64]
    float *const ssum = smax + kSlices * TB * kBlockStates;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b0 = blockIdx.x * TB;
    unsigned live = 0;                                                   // (the same in every thread)
#pragma unroll
    for (int g = 0; g < TB; ++g) {
        const int F = b0 + g < B ? fb::frames_of(frames, b0 + g, T) : 0;
        if (BACKWARD ? t < F - 1 : t < F) live |= 1u << g;
    }
    if (live == 0) return;

    // the previous rows of the live items, -inf behind state S - 1
#pragma unroll
    for (int g = 0; g < TB; ++g) {
        if (!(live >> g & 1)) continue;
        const float *v = BACKWARD ? vin + (size_t)(b0 + g) * Sp : post + ((size_t)(b0 + g) * T + (t - 1)) * S;
        for (int y = tid; y < Sp; y += kThreads) rows[g * Sp + y] = y < S ? v[y] : -INFINITY;
    }
    __syncthreads();

    // the lane's state against slice `wave` of y: quads [q_lo, q_hi)
    const int quads = (S + 3) / 4, per = slice_quads(S);
    const int q_lo = wave * per, q_hi = q_lo + per < quads ? q_lo + per : quads;
    float m[TB], s[TB];
#pragma unroll
    for (int g = 0; g < TB; ++g) {
        m[g] = -INFINITY;
        s[g] = 0.f;
    }
    if (q_lo < q_hi) {
        const float *col = P + (size_t)blockIdx.y * kBlockStates + lane;  // P[y][x]: y * Sp floats on (4 q + 3 < Sp)
        float p[4], next[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) p[c] = col[(size_t)(4 * q_lo + c) * Sp];
        for (int q = q_lo; q < q_hi; ++q) {
            const int qn = q + 1 < q_hi ? q + 1 : q_hi - 1;              // (past the slice: its last quad again)
#pragma unroll
            for (int c = 0; c < 4; ++c) next[c] = col[(size_t)(4 * qn + c) * Sp];
#pragma unroll
            for (int g = 0; g < TB; ++g) {
                if (!(live >> g & 1)) continue;
                const f4 v = *reinterpret_cast<const f4 *>(rows + g * Sp + 4 * q);
                float term[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) term[c] = p[c] + v[c];
                const float top = __builtin_fmaxf(__builtin_fmaxf(term[0], term[1]), __builtin_fmaxf(term[2], term[3]));
                const float now = __builtin_fmaxf(m[g], top), ref = ref_of(now);
                float sum = s[g] * ex2(m[g] - ref);
#pragma unroll
                for (int c = 0; c < 4; ++c) sum += ex2(term[c] - ref);   // (a NaN term loses the maximum and wins here)
                m[g] = now;
                s[g] = sum;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) p[c] = next[c];
        }
    }
#pragma unroll
    for (int g = 0; g < TB; ++g) {
        smax[(wave * TB + g) * kBlockStates + lane] = m[g];
        ssum[(wave * TB + g) * kBlockStates + lane] = s[g];
    }
    __syncthreads();

    // one thread per (state, item): the slices in their order
    for (int e = tid; e < TB * kBlockStates; e += kThreads) {
        const int g = e >> 6, x = blockIdx.y * kBlockStates + (e & 63);
        if (!(live >> g & 1) || x >= S) continue;
        float top = smax[e];
#pragma unroll
        for (int k = 1; k < kSlices; ++k) top = __builtin_fmaxf(top, smax[k * TB * kBlockStates + e]);
        const float ref = ref_of(top);
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < kSlices; ++k) sum += ssum[k * TB * kBlockStates + e] * ex2(smax[k * TB * kBlockStates + e] - ref);
        const float product = ref + lg2(sum);                            // (sum >= 1, or 0 with top = -inf, or NaN)
        if (BACKWARD) {
            yout[(size_t)(b0 + g) * Sp + x] = product;
        } else {
            const size_t at = ((size_t)(b0 + g) * T + t) * S + x;
            post[at] = obs[at] * kLog2e + product;
        }
    }
}

// ---- reductions over the states of an item: every thread ends with the same bits; `part` holds kWaves floats ----
__device__ __forceinline__ float block_max(float x, float *part) {
    x = fbl::wave_max(x);
    __syncthreads();                                                     // (the readers of the reduction before this one)
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
    __syncthreads();
    return fb::nan_max(fb::nan_max(part[0], part[1]), fb::nan_max(part[2], part[3]));
}
__device__ __forceinline__ float block_sum(float x, float *part) {
    x = fbb::wave_sum(x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

// ---- forward row t of item blockIdx.x: la_t = x_t - M_t in place, sum M_t, L at the item's last frame; zeros behind it ----
__global__ __launch_bounds__(kThreads) void fb_log_dense_forward_row_kernel(const float *__restrict__ obs,
                                                                            const int32_t *__restrict__ frames,
                                                                            const float *__restrict__ initial,
                                                                            float *__restrict__ post, float *__restrict__ loglik,
                                                                            double *__restrict__ Msum, int t, int T, int S) {
    __shared__ float part[kWaves];
    const int b = blockIdx.x, tid = threadIdx.x, F = fb::frames_of(frames, b, T);
    float *const row = post + ((size_t)b * T + t) * S;
    if (t >= F) {
        for (int j = tid; j < S; j += kThreads) row[j] = 0.f;
        return;
    }
    float top = -INFINITY;
    if (t == 0) {
        const float *o = obs + (size_t)b * T * S;
        for (int j = tid; j < S; j += kThreads) {
            const float x = (initial[j] + o[j]) * kLog2e;
            row[j] = x;
            top = fb::nan_max(top, x);
        }
    } else {
        for (int j = tid; j < S; j += kThreads) top = fb::nan_max(top, row[j]);
    }
    const float M = ref_of(block_max(top, part));
    float sum = 0.f;
    for (int j = tid; j < S; j += kThreads) {                            // (a thread reads what it wrote itself)
        const float la = row[j] - M;
        row[j] = la;
        sum += ex2(la);
    }
    double total = 0.;                                                   // thread 0 keeps sum M_t
    if (tid == 0) Msum[b] = total = (t == 0 ? 0. : Msum[b]) + (double)M;
    if (t < F - 1) return;
    const float Z = block_sum(sum, part);
    if (tid == 0) {
        const double L = (total + log2((double)Z)) * kLn2D;
        loglik[b] = (L != L || L == (double)INFINITY) ? NAN : (float)L;
    }
}

// ---- backward row t of item blockIdx.x: gamma_t over la_t in place, r_t to rout[b] (rows of Sp); y_t from yin[b] ----
__global__ __launch_bounds__(kThreads) void fb_log_dense_backward_row_kernel(const float *__restrict__ obs,
                                                                             const int32_t *__restrict__ frames,
                                                                             const float *__restrict__ loglik,
                                                                             const float *__restrict__ yin, float *__restrict__ post,
                                                                             float *__restrict__ rout, int t, int T, int S, int Sp) {
    __shared__ float part[kWaves];
    const int b = blockIdx.x, tid = threadIdx.x, F = fb::frames_of(frames, b, T);
    if (t >= F) return;
    const bool last = t == F - 1;
    const float *o = obs + ((size_t)b * T + t) * S, *y = yin + (size_t)b * Sp;
    float *const row = post + ((size_t)b * T + t) * S, *const r = rout + (size_t)b * Sp;
    float topq = -INFINITY, topr = -INFINITY;
    for (int j = tid; j < S; j += kThreads) {
        const float yj = last ? 0.f : y[j];
        topq = fb::nan_max(topq, row[j] + yj);
        topr = fb::nan_max(topr, o[j] * kLog2e + yj);
    }
    const float Q = ref_of(block_max(topq, part)), R = ref_of(block_max(topr, part));
    float sum = 0.f;
    for (int j = tid; j < S; j += kThreads) sum += ex2(row[j] + (last ? 0.f : y[j]) - Q);
    const float Zq = block_sum(sum, part);
    const bool finite = isfinite(loglik[b]);
    for (int j = tid; j < S; j += kThreads) {
        const float yj = last ? 0.f : y[j];
        const float e = ex2(row[j] + yj - Q);
        row[j] = finite ? e / Zq : NAN;
        r[j] = o[j] * kLog2e + yj - R;
    }
}

}  // namespace fbd
