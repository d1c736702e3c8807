// max_marginals.hpp -- max-marginals: the best path score through every frame and state (torbi_hip_max_marginals*,
// torbi_amd/margins.py, MARGINALS.md).
//
// All sums in float32 with one rounding each, A indexed [next][prev], F = batch_frames[b] clamped to [1, T]:
//     alpha_0[j] = fl(o_0[j] + pi[j])
//     alpha_t[j] = fl(o_t[j] + max_i fl(alpha_{t-1}[i] + A[j][i]))          1 <= t < F   (the decoder's posterior rows)
//     beta_{F-1}[i] = +0
//     beta_t[i]  = max_j fl(A[j][i] + fl(o_{t+1}[j] + beta_{t+1}[j]))       0 <= t < F-1
//     m_t[j]     = fl(alpha_t[j] + beta_t[j])   (t < F),    -inf   (F <= t < T)
//     score      = max_j alpha_{F-1}[j]
// A maximum of floats without NaN does not depend on the order it is taken in, so the values are the same whatever the
// tiling; only the sign of a zero may differ (m_{F-1} is stored as alpha_{F-1} itself, where the sum with +0 would turn a -0
// into +0).  -inf is an ordinary value.  An item that reads a NaN or +inf (its observation rows t < F, the initial vector, the
// matrix when F >= 2) gets NaN in every m_t, t < F, and a NaN score.  Sums of finite inputs that overflow float32 are outside
// the contract: such a +inf is no input, raises no alarm, and may meet a -inf as NaN.
//
// Dense route, per call: mm_prepare_kernel (the matrix transposed; its alarm), mm_first_kernel (frame 0), one
// mm_step_kernel<false> per frame 1 .. T-1 (alpha_t straight into marginals[b][t]), one mm_step_kernel<true> per frame
// T-2 .. 0 (beta_t into a two-row ping-pong, alpha_t turned into m_t in place), mm_final_kernel (score; NaN rows of an
// alarmed item).  2 (T - 1) step launches, no host synchronisation.
//
// The step kernel computes out[b][r] = max_c fl(M[r][c] + v[b][c]) for a tile of kItemTile items x kRowTile rows: 16 x 16
// lanes, each with a register block of kBI items x kBR rows; the contraction axis c goes through LDS in chunks of kChunk,
// the next chunk's operands in flight in registers while the current one is computed.  The cell is dense_forward.hpp's
// add, add, max3 per two values of c.  512 x 1440 outputs are 184 tiles, fewer than the chip has compute units, so a
// workgroup holds up to four such groups of lanes (step_groups): each takes its share of every chunk for the whole tile,
// and their maxima are merged through LDS once per launch -- the order of a maximum is free.  (An 8-row block per lane
// with eight groups of two waves reads a quarter less LDS per cell and measured 95.5 against 91.1 ms: MARGINALS.md.)
// The operand panel is read as Mt[c][r], r contiguous: the forward step (M = A, c = prev) reads the transposed copy of the
// workspace, the backward step (M = A^T, c = next) the caller's matrix itself.  Columns c >= S and items b >= B are staged
// as -inf.
//
// Uniform route (every matrix entry is u): max_i fl(x_i + u) = fl(max_i x_i + u), so with r_t = max_j o_t[j]
//     a_0 = max_j alpha_0[j],  c_t = fl(a_{t-1} + u),  a_t = fl(r_t + c_t),  alpha_t[j] = fl(o_t[j] + c_t)
//     beta_t = fl(u + fl(r_{t+1} + beta_{t+1}))   (one scalar per frame)
// mm_uniform_rows_kernel reduces every frame's r_t (a wave per row), mm_uniform_scan_kernel runs the 2 T scalars of an
// item (a lane per item: the chain is serial), mm_uniform_write_kernel writes m: the observation is read twice and the
// marginals written once.
//
// Workspace (mm::layout; nothing in it needs initialisation, the alarm words are cleared by every call):
//     dense:   at [S][S] fp32 the matrix transposed, beta [2][B][S] fp32, alarm [B + 1] int32 ([B]: the matrix)
//     uniform: rows [B][T] fp32 (r_t; a_0 at t = 0), c [B][T] fp32, beta [B][T] fp32, alarm [B + 1] int32
// No B * T * S region: alpha lives in the output.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "scratch.hpp"

namespace mm {

constexpr int kMaxStates = 16384;
constexpr int kThreads = 256;             // 16 x 16 lanes: one group of lanes that covers the whole output tile
constexpr int kBI = 4;                    // items per lane
constexpr int kBR = 4;                    // rows per lane
constexpr int kItemTile = 16 * kBI;       // 64 items per workgroup
constexpr int kRowTile = 16 * kBR;        // 64 rows per workgroup
constexpr int kChunk = 64;                // values of c per LDS stage
constexpr int kVStride = kItemTile + 4;   // LDS row of the v panel (float4 reads stay aligned)
constexpr int kMaxGroups = 4;             // groups of kThreads lanes that split a chunk's values of c among them
constexpr int kFullWaves = 2048;          // two waves on every SIMD of an MI355X: what a step launch tries to reach

// Groups per workgroup of a step launch over `tiles` output tiles: the fewest of 1, 2, 4 that bring the launch to kFullWaves
// waves (a group is four waves), else 4.  512 x 1440: 8 x 23 tiles, 4 groups.  A function of the shape alone.
__host__ __device__ inline int step_groups(long tiles) {
    int g = 1;
    while (g < kMaxGroups && tiles * 4 * g < kFullWaves) g *= 2;
    return g;
}

struct Layout {
    float *at, *beta;                     // dense
    float *rows, *c, *ubeta;              // uniform
    int32_t *alarm;
    size_t total;
};

// `base`: the caller's workspace aligned up to 256 bytes, or null for the byte count alone
inline Layout layout(char *base, int B, int T, int S, bool uniform) {
    Scratch a(base);
    Layout l{};
    if (uniform) {
        l.rows = a.take<float>((size_t)B * T);
        l.c = a.take<float>((size_t)B * T);
        l.ubeta = a.take<float>((size_t)B * T);
    } else {
        l.at = a.take<float>((size_t)S * S);
        l.beta = a.take<float>((size_t)2 * B * S);
    }
    l.alarm = a.take<int32_t>((size_t)B + 1);
    l.total = a.bytes + 256;              // (room to align the caller's base)
    return l;
}

__device__ __forceinline__ bool odd(float x) { return !(x < INFINITY); }     // NaN or +inf
__device__ __forceinline__ int clamp_frames(int f, int T) { return f < 1 ? 1 : (f > T ? T : f); }

// at[i][j] = A[j][i]; alarm[B] raised if the matrix holds a NaN or +inf
__global__ __launch_bounds__(256) void mm_prepare_kernel(const float *__restrict__ A, float *__restrict__ at,
                                                         int32_t *__restrict__ matrix_alarm, int S) {
    __shared__ float tile[32][33];
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
    const int i0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
    bool bad = false;
    for (int r = y; r < 32; r += 8) {
        const int j = j0 + r, i = i0 + x;
        float a = 0.f;
        if (j < S && i < S) {
            a = A[(size_t)j * S + i];
            bad |= odd(a);
        }
        tile[r][x] = a;
    }
    __syncthreads();
    for (int r = y; r < 32; r += 8) {
        const int i = i0 + r, j = j0 + x;
        if (i < S && j < S) at[(size_t)i * S + j] = tile[x][r];
    }
    if (bad) *matrix_alarm = 1;
}

// frame 0: alpha_0[j] = fl(o_0[j] + pi[j]); grid (B, ceil(S / 256))
__global__ __launch_bounds__(256) void mm_first_kernel(const float *__restrict__ obs, const float *__restrict__ initial,
                                                       float *__restrict__ marg, int32_t *__restrict__ alarm, int T, int S) {
    const int b = blockIdx.x;
    const int j = blockIdx.y * 256 + threadIdx.x;
    if (j >= S) return;
    const float o = obs[(size_t)b * T * S + j], p = initial[j];
    if (odd(o) || odd(p)) alarm[b] = 1;
    marg[(size_t)b * T * S + j] = o + p;
}

// One frame of one pass.  grid (ceil(B / kItemTile), ceil(S / kRowTile)), block kThreads * KG.
//   forward  (t >= 1):    v[b][c] = alpha_{t-1}[b][c] = marg[b][t-1][c], mt = at;
//                         marg[b][t][r] = fl(o_t[r] + out) for t < F, -inf for t >= F
//   backward (t <= T-2):  v[b][c] = fl(o_{t+1}[c] + beta_{t+1}[b][c]) (beta_{F-1} = +0), mt = A;
//                         for t < F-1: beta_t[b][r] = out, marg[b][t][r] = fl(marg[b][t][r] + out); nothing for t >= F-1
// beta: [2][B][S], frame t in plane t & 1.  Every thread stages; group g of the KG groups takes the values of c
// [g, g + 1) * kChunk / KG of every chunk for the whole tile, and the groups' maxima meet in LDS behind the last chunk, one group after the other.
template <bool BACKWARD, int KG>
__global__ __launch_bounds__(kThreads * KG) void mm_step_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                                const float *__restrict__ mt, float *__restrict__ marg,
                                                                float *__restrict__ beta, int32_t *__restrict__ alarm, int t,
                                                                int B, int T, int S) {
    constexpr int NT = kThreads * KG;
    constexpr int MP = kChunk * kRowTile / NT;         // staging passes of a thread over the M panel ...
    constexpr int VP = kChunk * kItemTile / NT;        // ... and over the v panel
    constexpr int CG = kChunk / KG;                    // values of c per group and chunk
    __shared__ __attribute__((aligned(16))) float ms[kChunk][kRowTile];
    __shared__ __attribute__((aligned(16))) float vs[kChunk][kVStride];
    __shared__ int fs[kItemTile];
    const int tid = threadIdx.x;
    const int group = tid / kThreads, lt = tid % kThreads;            // (a group is four whole waves)
    const int b0 = blockIdx.x * kItemTile, r0 = blockIdx.y * kRowTile;
    // an item takes part in the contraction while its output is a recurrence value: t < F (forward), t < F-1 (backward)
    const int last = BACKWARD ? t + 1 : t;
    bool live = false;
    if (tid < kItemTile) {
        const int b = b0 + tid;
        const int f = b < B ? clamp_frames(frames[b], T) : 0;
        fs[tid] = f;
        live = last < f;
    }
    const bool any = __syncthreads_or(live);       // (also publishes fs)

    float acc[kBI][kBR];
#pragma unroll
    for (int i = 0; i < kBI; ++i)
#pragma unroll
        for (int r = 0; r < kBR; ++r) acc[i][r] = -INFINITY;

    const int rx = lt & 15, bx = lt >> 4;
    if (any) {
        // staging: the M panel as 64 rows x NT / 64 values of c per pass, the v panel as 64 values of c x NT / 64 items per pass
        const int mr = tid & 63, mc = tid >> 6;
        const int vc = tid & 63, vb = tid >> 6;
        const bool row_ok = r0 + mr < S;
        float pm[MP], pv[VP];
        const size_t plane = (size_t)B * S;
        auto fetch = [&](int c0) {
#pragma unroll
            for (int p = 0; p < MP; ++p) {
                const int c = c0 + mc + (NT / 64) * p;
                pm[p] = (row_ok && c < S) ? mt[(size_t)c * S + r0 + mr] : -INFINITY;
            }
            const int c = c0 + vc;
#pragma unroll
            for (int p = 0; p < VP; ++p) {
                const int ib = vb + (NT / 64) * p, b = b0 + ib;
                const int f = fs[ib];
                float v = -INFINITY;
                if (c < S && last < f) {
                    if (BACKWARD) {
                        const float o = obs[((size_t)b * T + (t + 1)) * S + c];
                        const float be = (t + 1 == f - 1) ? 0.f : beta[(size_t)((t + 1) & 1) * plane + (size_t)b * S + c];
                        v = o + be;
                    } else {
                        v = marg[((size_t)b * T + (t - 1)) * S + c];
                    }
                }
                pv[p] = v;
            }
        };
        fetch(0);
        for (int c0 = 0; c0 < S; c0 += kChunk) {
#pragma unroll
            for (int p = 0; p < MP; ++p) ms[mc + (NT / 64) * p][mr] = pm[p];
#pragma unroll
            for (int p = 0; p < VP; ++p) vs[vc][vb + (NT / 64) * p] = pv[p];
            __syncthreads();
            if (c0 + kChunk < S) fetch(c0 + kChunk);
#pragma unroll 4
            for (int c = group * CG; c < group * CG + CG; c += 2) {
                const float4 m0 = *reinterpret_cast<const float4 *>(&ms[c][4 * rx]);
                const float4 v0 = *reinterpret_cast<const float4 *>(&vs[c][4 * bx]);
                const float4 m1 = *reinterpret_cast<const float4 *>(&ms[c + 1][4 * rx]);
                const float4 v1 = *reinterpret_cast<const float4 *>(&vs[c + 1][4 * bx]);
                const float ma[2][4] = {{m0.x, m0.y, m0.z, m0.w}, {m1.x, m1.y, m1.z, m1.w}};
                const float va[2][4] = {{v0.x, v0.y, v0.z, v0.w}, {v1.x, v1.y, v1.z, v1.w}};
#pragma unroll
                for (int i = 0; i < kBI; ++i)
#pragma unroll
                    for (int r = 0; r < kBR; ++r)
                        acc[i][r] = fmaxf(fmaxf(acc[i][r], ma[0][r] + va[0][i]), ma[1][r] + va[1][i]);      // add, add, max3
            }
            __syncthreads();
        }
        if (KG > 1) {                              // (the M panel is free behind the last chunk's barrier: kChunk x kRowTile floats
            float *const merge = &ms[0][0];        //  hold one group's kBI x kBR maxima of its kThreads lanes)
            static_assert(kChunk * kRowTile >= kBI * kBR * kThreads, "the merge buffer is the M panel");
            for (int g = 1; g < KG; ++g) {
                if (group == g) {
#pragma unroll
                    for (int i = 0; i < kBI; ++i)
#pragma unroll
                        for (int r = 0; r < kBR; ++r) merge[(i * kBR + r) * kThreads + lt] = acc[i][r];
                }
                __syncthreads();
                if (group == 0) {
#pragma unroll
                    for (int i = 0; i < kBI; ++i)
#pragma unroll
                        for (int r = 0; r < kBR; ++r) acc[i][r] = fmaxf(acc[i][r], merge[(i * kBR + r) * kThreads + lt]);
                }
                __syncthreads();
            }
        }
    }
    if (group > 0) return;

#pragma unroll
    for (int i = 0; i < kBI; ++i) {
        const int ib = 4 * bx + i, b = b0 + ib;
        if (b >= B) continue;
        const int f = fs[ib];
        bool seen = false;
#pragma unroll
        for (int r = 0; r < kBR; ++r) {
            const int j = r0 + 4 * rx + r;
            if (j >= S) continue;
            const size_t at_ = ((size_t)b * T + t) * S + j;
            if (BACKWARD) {
                if (t < f - 1) {
                    beta[(size_t)(t & 1) * (size_t)B * S + (size_t)b * S + j] = acc[i][r];
                    marg[at_] = marg[at_] + acc[i][r];
                }
            } else if (t < f) {
                const float o = obs[at_];
                seen |= odd(o);
                marg[at_] = o + acc[i][r];
            } else {
                marg[at_] = -INFINITY;
            }
        }
        if (seen) alarm[b] = 1;
    }
}

// score = max_j alpha_{F-1}[j] (row F-1 of the marginals holds alpha_{F-1} itself); an alarmed item gets NaN in its rows
// t < F and a NaN score.  grid (B), block 256.
__global__ __launch_bounds__(256) void mm_final_kernel(const int32_t *__restrict__ frames, const int32_t *__restrict__ alarm,
                                                       float *__restrict__ marg, float *__restrict__ scores, int B, int T, int S) {
    __shared__ float part[4];
    const int b = blockIdx.x;
    const int f = clamp_frames(frames[b], T);
    float *const item = marg + (size_t)b * T * S;
    if (alarm[b] != 0 || (alarm[B] != 0 && f >= 2)) {
        const size_t n = (size_t)f * S;
        for (size_t e = threadIdx.x; e < n; e += 256) item[e] = NAN;
        if (threadIdx.x == 0) scores[b] = NAN;
        return;
    }
    float best = -INFINITY;
    for (int j = threadIdx.x; j < S; j += 256) best = fmaxf(best, item[(size_t)(f - 1) * S + j]);
    for (int d = 32; d >= 1; d >>= 1) best = fmaxf(best, __shfl_xor(best, d));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) scores[b] = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

// ---- the uniform route ----

// rows[b][t] = max_j o_t[j] for 1 <= t < F, rows[b][0] = max_j fl(o_0[j] + pi[j]); the item's alarm.  A wave per row,
// 4 rows per workgroup; grid (ceil(B * T / 4)).
template <bool VEC>
__global__ __launch_bounds__(256) void mm_uniform_rows_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                              const float *__restrict__ initial, float *__restrict__ rows,
                                                              int32_t *__restrict__ alarm, int B, int T, int S) {
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (size_t)B * T) return;
    const int b = (int)(row / T), t = (int)(row - (size_t)b * T);
    if (t >= clamp_frames(frames[b], T)) return;
    const int lane = threadIdx.x & 63;
    const float *const o = obs + row * S;
    float best = -INFINITY;
    bool seen = false;
    if (VEC) {
        const float4 *const o4 = reinterpret_cast<const float4 *>(o);
        const float4 *const p4 = reinterpret_cast<const float4 *>(initial);
        for (int q = lane; q < S / 4; q += 64) {
            float4 x = o4[q];
            seen |= odd(x.x) || odd(x.y) || odd(x.z) || odd(x.w);
            if (t == 0) {
                const float4 p = p4[q];
                seen |= odd(p.x) || odd(p.y) || odd(p.z) || odd(p.w);
                x.x += p.x; x.y += p.y; x.z += p.z; x.w += p.w;
            }
            best = fmaxf(fmaxf(best, fmaxf(x.x, x.y)), fmaxf(x.z, x.w));
        }
    } else {
        for (int j = lane; j < S; j += 64) {
            float x = o[j];
            seen |= odd(x);
            if (t == 0) {
                const float p = initial[j];
                seen |= odd(p);
                x += p;
            }
            best = fmaxf(best, x);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) best = fmaxf(best, __shfl_xor(best, d));
    if (__any(seen) && lane == 0) alarm[b] = 1;
    if (lane == 0) rows[row] = best;
}

// The 2 T scalars of an item and its score, a lane per item (each chain is serial: no sum here is associative).
// `model_bad`: the uniform value itself is NaN or +inf.  grid (ceil(B / 64)), block 64.
__global__ __launch_bounds__(64) void mm_uniform_scan_kernel(const int32_t *__restrict__ frames, const float *__restrict__ rows,
                                                             float *__restrict__ cs, float *__restrict__ bs,
                                                             int32_t *__restrict__ alarm, float *__restrict__ scores, float u,
                                                             int model_bad, int B, int T) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int f = clamp_frames(frames[b], T);
    const size_t at_ = (size_t)b * T;
    if (model_bad && f >= 2) alarm[b] = 1;
    const bool bad = alarm[b] != 0 || (model_bad && f >= 2);
    float a = rows[at_];
    cs[at_] = 0.f;
    for (int t = 1; t < f; ++t) {
        const float c = a + u;
        cs[at_ + t] = c;
        a = rows[at_ + t] + c;
    }
    scores[b] = bad ? NAN : a;
    float be = 0.f;
    bs[at_ + f - 1] = 0.f;
    for (int t = f - 2; t >= 0; --t) {
        be = u + (rows[at_ + t + 1] + be);
        bs[at_ + t] = be;
    }
}

// m_t[j] = fl(fl(o_t[j] + c_t) + beta_t) (t = 0: pi[j] in place of c_t; t = F-1: alpha itself); -inf for t >= F; NaN in the
// rows t < F of an alarmed item.  One element (VEC: four) per thread and pass; grid-stride.
template <bool VEC>
__global__ __launch_bounds__(256) void mm_uniform_write_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                               const float *__restrict__ initial, const float *__restrict__ cs,
                                                               const float *__restrict__ bs, const int32_t *__restrict__ alarm,
                                                               float *__restrict__ marg, int B, int T, int S) {
    constexpr int W = VEC ? 4 : 1;
    const size_t n = (size_t)B * T * S / W;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const size_t row = e * W / S;
        const int j = (int)(e * W - row * S);
        const int b = (int)(row / T), t = (int)(row - (size_t)b * T);
        const int f = clamp_frames(frames[b], T);
        float x[W];
        if (t >= f) {
#pragma unroll
            for (int q = 0; q < W; ++q) x[q] = -INFINITY;
        } else if (alarm[b] != 0) {
#pragma unroll
            for (int q = 0; q < W; ++q) x[q] = NAN;
        } else {
            const float c = cs[row], be = bs[row];
            if (VEC) {
                const float4 o = *reinterpret_cast<const float4 *>(obs + e * 4);
                x[0] = o.x; x[1 % W] = o.y; x[2 % W] = o.z; x[3 % W] = o.w;
            } else {
                x[0] = obs[e];
            }
#pragma unroll
            for (int q = 0; q < W; ++q) {
                const float alpha = x[q] + (t == 0 ? initial[j + q] : c);
                x[q] = t == f - 1 ? alpha : alpha + be;
            }
        }
        if (VEC) {
            *reinterpret_cast<float4 *>(marg + e * 4) = make_float4(x[0], x[1 % W], x[2 % W], x[3 % W]);
        } else {
            marg[e] = x[0];
        }
    }
}

}  // namespace mm
