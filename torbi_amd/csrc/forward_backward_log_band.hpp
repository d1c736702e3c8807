// forward_backward_log_band.hpp -- state posteriors and log-likelihood in LOG SPACE for a transition matrix that holds ONE
// value outside a band of up to 512 entries (torbi_hip_forward_backward_log_band, torbi_amd/posterior.py
// forward_backward_log_banded, POSTERIOR.md "Log-space band route").
//
// Every other forward-backward kernel runs the scaled recurrence a_t = e_t (E a_{t-1}) / c_{t-1} in float32: a filtered row
// that spans more than float32's range loses the states that would win later.  This one keeps every row as logarithms, each
// row normalised by its own maximum (natural logs in the contract, A [next][prev]):
//     x_0 = pi + o_0                                   M_t = max_j x_t[j]   (-inf read as 0, NaN propagates)
//     x_t[j] = o_t[j] + lse_i (A[j,i] + la_{t-1}[i])   la_t = x_t - M_t
//     L = sum_{t<F} M_t (fp64) + lse_j la_{F-1}[j]
//     y_t[i] = lse_j (A[j,i] + r_{t+1}[j])             r_t = o_t + y_t - max_j (o_t + y_t),   y_{F-1} = 0
//     gamma_t = softmax_j (la_t[j] + y_t[j])           (the row's own maximum and sum)
// (r_t is o_t + lb_t up to a constant of the row, which the softmax and the next row's own maximum take out again: the
// backward row needs one normalisation, not two.)  The band split stays "band minus constant, constant over everything":
//     lse_i (A[j,i] + v[i]) = lse( lse_{i in band(j)} (D[j,i] + v[i]),  background + lse_i v[i] )
//     D = A + log1p(-exp(background - A))      (fp64, rounded once; -inf where A == background; D = A for -inf outside)
// lse_i v[i] is one sum per item and frame over values whose maximum is 0.  An in-band entry below a finite background would
// be a negative weight and counts as a broken promise.
//
// Inside the launch rows and pack are in BASE-2 logarithms (v_exp_f32 and v_log_f32 are base 2): the observation is scaled
// by log2(e) where it is loaded, L by ln 2 where it is stored.
//
// Launches: pack (with the flag reset), verify, then ONE launch that runs every frame of both passes; a workgroup of 1024
// threads owns G whole items, nothing waits across workgroups.  The pack order, the plan (blocks, slices, dquads, LDS row
// stride) and the way a lane walks the band are forward_backward_wide_band.hpp's: a lane owns 4 consecutive states x G
// items, one 16-byte piece of the LDS row window serves 16 terms.  Clipped and padding positions of the pack and the halo
// of the rows hold -inf.
//
// Band sum of one (state, item): a blocked running maximum.  Per dquad the 4 terms of a state are formed (one add each),
// their maximum joins the running one, the running sum is rescaled by ONE exponential and every term adds one: 1.25
// exponentials per term, the band is read once.  The running maximum is the state's own -- a maximum shared by the 4 states
// of a lane would save 0.19 exponentials per term and flush a state whose band sum lies 2^126 under its neighbour's, which
// is the blind spot this route exists to close.  A reference of -inf is read as 0, so no -inf - -inf arises.
//
// A frame: phase A (the slices' (m, s) pairs to LDS), then phase B with one thread per state (tid, tid + 1024, ...):
//   forward   slices combined in slice order, background term, observation: x to the row in place | row maximum |
//             la to the row and to `posterior` in place, sum of exp2(la) | next frame
//   backward  y from the slices; q = la + y beside the slices, o + y to the row | both maxima | exp2(q - Q) and its sum,
//             r to the row and its sum | gamma = exp2(q - Q) / sum in place | next frame
// Reductions: 64-lane butterfly, 16 wave values in LDS, 16-lane butterfly: every thread holds the same bits, and thread 0
// keeps sum M_t in fp64 in LDS.  Workspace: two packs and one flag, no (B, T) and no (B, T, S) region.
//
// The order of every operation of an item is fixed by (S, band) alone: an item's bits depend neither on G nor on its tile
// nor on the batch.  No float atomics, vector stores only.
#pragma once

#include "forward_backward_wide_band.hpp"

namespace fbl {

using fbw::f4;
using fbw::Plan;
using fbw::barrier;
constexpr int kThreads = fbw::kThreads, kWaves = fbw::kWaves;
constexpr int kMaxStates = fbw::kMaxStates, kMaxWindow = fbw::kMaxWindow, kMaxGroup = 4;
constexpr int kMaxLdsBytes = fbw::kMaxLdsBytes;
constexpr int kBlockStates = fbw::kBlockStates;
constexpr int kParts = 5;                    // wave values of a frame: row max, row sum; backward max q, max r, sum q (sum r: row sum)
constexpr float kLog2e = 1.4426950408889634f;
constexpr double kLog2eD = 1.4426950408889634074, kLn2D = 0.69314718055994530942;

struct Layout : Plan { float *P[2]; int32_t *flag; size_t total; };

// `base`: the caller's workspace aligned up to 256 bytes, or null for the byte count alone
inline Layout layout(char *base, int S, int reach_left, int reach_right) {
    Layout l;
    static_cast<Plan &>(l) = fbw::plan_of(S, reach_left, reach_right);
    Scratch a(base);
    l.P[0] = a.take<float>(fbw::pack_floats(l, 0));
    l.P[1] = a.take<float>(fbw::pack_floats(l, 1));
    l.flag = a.take<int32_t>(1);
    l.total = a.bytes + 256;                 // (room to align the caller's base)
    return l;
}

// LDS of a tile of G items: the head (what thread 0 keeps of every item: sum M_t in fp64, Z_{F-1}, L), rows [G][stride]; slice
// maxima and slice sums [KS][G][S4] each; wave values [kParts][G][16]
constexpr int kHeadBytes = kMaxGroup * 16;
__host__ __device__ inline size_t lds_bytes(int G, const Plan &p) {
    return kHeadBytes + (size_t)G * 4 * ((size_t)p.stride + 2 * (size_t)p.slices * p.S4 + kParts * kWaves);
}

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }     // v_exp_f32
__device__ __forceinline__ float lg2(float x) { return __builtin_amdgcn_logf(x); }      // v_log_f32
// what a difference is taken against: a maximum, with -inf read as 0
__device__ __forceinline__ float ref_of(float m) { return m == -INFINITY ? 0.f : m; }
// log2(2^a + 2^b)
__device__ __forceinline__ float lse2(float a, float b) {
    const float r = ref_of(fb::nan_max(a, b));
    return r + lg2(ex2(a - r) + ex2(b - r));
}

// ---- both packs of D in base 2; resets the promise flag.  grid (blocks * max Dq, 2 passes), block 256 = 4 diagonals x 64 lanes ----
__global__ __launch_bounds__(256) void fb_log_pack_kernel(const float *__restrict__ A, float *__restrict__ Pf,
                                                          float *__restrict__ Pb, int32_t *__restrict__ flag, float background,
                                                          Plan p, int S) {
    const int pass = blockIdx.y, Dq = p.Dq[pass], most = p.Dq[0] > p.Dq[1] ? p.Dq[0] : p.Dq[1];
    if (blockIdx.x == 0 && pass == 0 && threadIdx.x == 0) *flag = 0;
    const int blk = (int)blockIdx.x / most, q = (int)blockIdx.x - blk * most;
    if (q >= Dq) return;
    const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = 4 * q + c - (p.left4[pass] - p.left[pass]);            // the diagonal of the band, 0 <= k < W
    float v[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int x = kBlockStates * blk + 4 * lane + n, y = x - p.left[pass] + k;   // output state, input state
        const bool in = k >= 0 && k < p.W && x < S && y >= 0 && y < S;
        const size_t at = pass == 0 ? (size_t)x * S + y : (size_t)y * S + x;         // A [next][prev]
        float d = -INFINITY;
        if (in) {
            const float a = A[at];
            if (background == -INFINITY) d = (float)((double)a * kLog2eD);
            else if (a != background) d = (float)(((double)a + log1p(-exp((double)background - (double)a))) * kLog2eD);
        }
        v[n] = d;
    }
    f4 *out = reinterpret_cast<f4 *>(pass == 0 ? Pf : Pb);
    out[(((size_t)blk * Dq + q) * 4 + c) * 64 + lane] = f4{v[0], v[1], v[2], v[3]};
}

// ---- the promise: every entry outside the band equals `background` bit for bit, none inside lies under a finite one; one
// wave per matrix row ----
__global__ __launch_bounds__(64) void fb_log_verify_kernel(const float *__restrict__ A, int32_t *__restrict__ flag,
                                                           float background, int reach_left, int reach_right, int S) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const float *row = A + (size_t)j * S;
    bool broken = banddiag::stray_in_row(row, j, reach_left, reach_right, S, __float_as_uint(background), lane, 64);
    const int lo = j - reach_left < 0 ? 0 : j - reach_left, hi = j + reach_right > S - 1 ? S - 1 : j + reach_right;
    for (int i = lo + lane; i <= hi; i += 64) broken = broken || row[i] < background;
    if (broken) *flag = 1;
}

// `passes` = 1: the forward pack alone (a forward-only caller; P[1] is not written)
inline hipError_t pack_and_verify(const float *A, const Layout &l, float background, int S, hipStream_t st, int passes = 2) {
    const int most = l.Dq[0] > l.Dq[1] ? l.Dq[0] : l.Dq[1];
    hipLaunchKernelGGL(fb_log_pack_kernel, dim3((unsigned)(l.blocks * most), passes), dim3(256), 0, st, A, l.P[0], l.P[1], l.flag,
                       background, static_cast<const Plan &>(l), S);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fb_log_verify_kernel, dim3(S), dim3(64), 0, st, A, l.flag, background, l.reach_left, l.reach_right, S);
    return hipGetLastError();
}

// One tile in the dynamic LDS of a workgroup, and the frames of its items
template <int G>
struct Tile {
    double *Msum;                            // [kMaxGroup] sum of M_t, thread 0's
    float *Zlast, *L;                        // [kMaxGroup] Z_{F-1}; L as the caller gets it
    float *rows, *smax, *ssum, *part;        // [G][stride]; [KS][G][S4] twice; [kParts][G][16]
    int b0, Fmax, F[G];
    __device__ __forceinline__ Tile(unsigned char *lds, const Plan &p) {
        Msum = reinterpret_cast<double *>(lds);
        Zlast = reinterpret_cast<float *>(Msum + kMaxGroup);
        L = Zlast + kMaxGroup;
        rows = reinterpret_cast<float *>(lds + kHeadBytes);
        smax = rows + (size_t)G * p.stride;
        ssum = smax + (size_t)p.slices * G * p.S4;
        part = ssum + (size_t)p.slices * G * p.S4;
    }
};

// Whether a lane keeps, beside the dquad of band it reads, the next one in flight, and of every item's row window the upper
// piece for the next dquad: with up to 2 items.  With 4 the 32 registers of both would not fit the 128 VGPRs of a lane at 16
// waves; the 320 exponentials of a dquad cover its load, and the second LDS read is one per 80.
constexpr bool keeps_ahead(int G) { return G <= 2; }

// ---- phase A of one lane: for its 4 states n and every item g, (m, s) with 2^m * s = sum over the dquads [q_lo, q_hi) and
// their diagonals c of 2^(P[q][c][n] + row_g[4 q + c + n]) ----
// `pack`: the lane's first piece of its block (piece (q, c) 64 (4 q + c) f4 on); `row`: item 0's row at the lane's first
// state (item g: g * stride floats on).  q_lo < q_hi, both the same in every lane of the wave.
template <int G>
__device__ __forceinline__ void band_lse(const f4 *__restrict__ pack, const float *row, int stride, int q_lo, int q_hi,
                                         float (&m)[G][4], float (&s)[G][4]) {
    constexpr bool kAhead = keeps_ahead(G);
    f4 band[4], next[4], lo[kAhead ? G : 1];
#pragma unroll
    for (int c = 0; c < 4; ++c) band[c] = pack[(size_t)(4 * q_lo + c) * 64];
    if (kAhead) {
#pragma unroll
        for (int g = 0; g < G; ++g) lo[g] = *reinterpret_cast<const f4 *>(row + g * stride + 4 * q_lo);
    }
    for (int q = q_lo; q < q_hi; ++q) {
        const int qn = q + 1 < q_hi ? q + 1 : q_hi - 1;                  // (past the slice: its last dquad again)
        if (kAhead) {
#pragma unroll
            for (int c = 0; c < 4; ++c) next[c] = pack[(size_t)(4 * qn + c) * 64];
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const f4 low = kAhead ? lo[g] : *reinterpret_cast<const f4 *>(row + g * stride + 4 * q);
            const f4 hi = *reinterpret_cast<const f4 *>(row + g * stride + 4 * q + 4);
            const float v[8] = {low.x, low.y, low.z, low.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                float term[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) term[c] = band[c][n] + v[n + c];
                const float top = __builtin_fmaxf(__builtin_fmaxf(term[0], term[1]), __builtin_fmaxf(term[2], term[3]));
                const float now = __builtin_fmaxf(m[g][n], top), ref = ref_of(now);
                float sum = s[g][n] * ex2(m[g][n] - ref);
#pragma unroll
                for (int c = 0; c < 4; ++c) sum += ex2(term[c] - ref);   // (a NaN term loses the maximum and wins here)
                m[g][n] = now;
                s[g][n] = sum;
            }
            if (kAhead) lo[g] = hi;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) band[c] = kAhead ? next[c] : pack[(size_t)(4 * qn + c) * 64];
    }
}

// phase A of the workgroup for one pass: every owning wave's slice pairs to tile.smax / tile.ssum (the caller's barrier follows)
template <int G>
__device__ __forceinline__ void band_phase(const Tile<G> &tile, const Plan &p, int pass, const float *__restrict__ P, int S) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave >= p.blocks * p.slices) return;
    const int blk = wave % p.blocks, sl = wave / p.blocks, Dq = p.Dq[pass];
    const int per = (Dq + p.slices - 1) / p.slices;
    const int q_lo = sl * per, q_hi = q_lo + per < Dq ? q_lo + per : Dq;
    const int x0 = kBlockStates * blk + 4 * lane;
    if (x0 >= S) return;
    float m[G][4], s[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            m[g][n] = -INFINITY;
            s[g][n] = 0.f;
        }
    if (q_lo < q_hi)
        band_lse<G>(reinterpret_cast<const f4 *>(P) + (size_t)blk * Dq * 256 + lane, tile.rows + x0, p.stride, q_lo, q_hi, m, s);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const size_t at = ((size_t)sl * G + g) * p.S4 + x0;
        *reinterpret_cast<f4 *>(tile.smax + at) = f4{m[g][0], m[g][1], m[g][2], m[g][3]};
        *reinterpret_cast<f4 *>(tile.ssum + at) = f4{s[g][0], s[g][1], s[g][2], s[g][3]};
    }
}

// log2 of the whole product for state j of item g: the slices in their order, then the constant outside the band times the
// operand's sum (`outside` = background in base 2 + log2 of that sum; unused where the background is -inf)
template <int G>
__device__ __forceinline__ float product_of(const Tile<G> &tile, const Plan &p, int g, int j, bool finite, float outside) {
    float m = tile.smax[(size_t)g * p.S4 + j];
    for (int k = 1; k < p.slices; ++k) m = __builtin_fmaxf(m, tile.smax[((size_t)k * G + g) * p.S4 + j]);
    const float ref = ref_of(m);
    float s = 0.f;
    for (int k = 0; k < p.slices; ++k) {
        const size_t at = ((size_t)k * G + g) * p.S4 + j;
        s += tile.ssum[at] * ex2(tile.smax[at] - ref);
    }
    const float band = ref + lg2(s);                                     // (s >= 1, or 0 with m = -inf, or NaN)
    return finite ? lse2(band, outside) : band;
}

// ---- reductions over the states of an item: every thread ends with the same bits ----
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = fb::nan_max(x, __shfl_xor(x, off, 64));
    return x;
}
__device__ __forceinline__ float max16(float x) {
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) x = fb::nan_max(x, __shfl_xor(x, off, 64));
    return x;
}
// a thread's share of G values to slot `which` of the wave values (the caller's barrier follows)
template <int G, bool MAX>
__device__ __forceinline__ void to_waves(const Tile<G> &tile, int which, const float (&x)[G]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float a = MAX ? wave_max(x[g]) : fbb::wave_sum(x[g]);
        if (lane == 0) tile.part[((size_t)which * G + g) * kWaves + wave] = a;
    }
}
template <int G, bool MAX>
__device__ __forceinline__ void from_waves(const Tile<G> &tile, int which, float (&x)[G]) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float a = tile.part[((size_t)which * G + g) * kWaves + (threadIdx.x & 15)];
        x[g] = MAX ? max16(a) : fbb::sum16(a);
    }
}

// What the OPS arm of the kernel leaves for the counts (counts_log_band.hpp), all in base-2 logs; rows t >= F_b are never
// written:
//     LAop[b][t][i] = la_t[i]                                          rows of S4 floats (the backward pass overwrites `post`)
//     Mrow[b][t]    = M_t
//     Wop[b][t][j]  = o_t[j] log2e + y_t[j] - (M_t + Q_t + log2 sum_j 2^(q_t[j] - Q_t))      q_t = la_t + y_t, Q_t its maximum
// so that xi_t(j, i) = 2^(A[j,i] log2e + LAop[t-1][i] + Wop[t][j]): la_{t-1} and y_t stand for alpha_{t-1} and beta_t up to
// constants of their rows, gamma_t[j] = 2^(q_t[j] - Q_t) / sum fixes the product of both constants against the likelihood at
// frame t, and the rows t - 1 and t differ by M_t.  Summed over i it is gamma_t[j].
struct Operands { float *LAop, *Wop, *Mrow; };

// ---- both passes of G items per workgroup; grid ceil(B / G), dynamic LDS lds_bytes(G, plan).  OPS: also the operand rows
// above; `false` is the kernel as it was, and `true` adds stores and touches no value that `false` computes ----
template <int G, bool OPS = false>
__global__ __launch_bounds__(kThreads) void fb_log_band_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                               const float *__restrict__ initial, const float *__restrict__ Pf,
                                                               const float *__restrict__ Pb, const int32_t *__restrict__ flag,
                                                               float *__restrict__ post, float *__restrict__ loglik,
                                                               float background, Plan p, int B, int T, int S,
                                                               Operands ops = Operands{nullptr, nullptr, nullptr}) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Tile<G> tile(lds_raw, p);
    const int tid = threadIdx.x, stride = p.stride;
    const bool finite = background != -INFINITY;
    const float bg2 = background * kLog2e;
    const int b0 = tile.b0 = blockIdx.x * G;
    int Fmax = 1;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        tile.F[g] = b0 + g < B ? fb::frames_of(frames, b0 + g, T) : 0;   // (0: an item beyond the batch never takes a step)
        Fmax = tile.F[g] > Fmax ? tile.F[g] : Fmax;
    }
    const int *F = tile.F;
    float *const rows = tile.rows;
    for (int e = tid; e < G * stride; e += kThreads) rows[e] = -INFINITY;        // (the halos stay -inf all pass long)
#pragma unroll
    for (int g = 0; g < G; ++g) {                                                // rows an item does not have
        if (b0 + g >= B) continue;
        float *out = post + (size_t)(b0 + g) * T * S;
        for (size_t e = (size_t)F[g] * S + tid; e < (size_t)T * S; e += kThreads) out[e] = 0.f;
    }
    barrier();

    // ---- forward: la_t to the row and to `post`; M_t summed in fp64 (every thread holds the same M_t: thread 0 keeps the
    // sum, in LDS, as nothing of an item lives in registers over phase A); Z_t = sum_j 2^la_t[j] stays in the wave values ----
    if (tid < G) {
        tile.Msum[tid] = 0.;
        tile.Zlast[tid] = 0.f;
    }
    {
        float *const cur = rows + p.left4[0];
        for (int t = 0; t < Fmax; ++t) {
            if (t > 0) {
                band_phase(tile, p, 0, Pf, S);
                barrier();
            }
            float top[G], outside[G];
            if (t > 0) from_waves<G, false>(tile, 1, outside);                   // Z_{t-1}
#pragma unroll
            for (int g = 0; g < G; ++g) {
                top[g] = -INFINITY;
                outside[g] = finite && t > 0 ? bg2 + lg2(outside[g]) : 0.f;
            }
            for (int j = tid; j < S; j += kThreads)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (t >= F[g]) continue;
                    const float o = obs[((size_t)(b0 + g) * T + t) * S + j];
                    const float x = t == 0 ? (initial[j] + o) * kLog2e : o * kLog2e + product_of(tile, p, g, j, finite, outside[g]);
                    cur[g * stride + j] = x;
                    top[g] = fb::nan_max(top[g], x);
                }
            to_waves<G, true>(tile, 0, top);
            barrier();
            from_waves<G, true>(tile, 0, top);
            float sum[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                top[g] = ref_of(top[g]);
                if (tid == 0 && t < F[g]) tile.Msum[g] += (double)top[g];
                if (OPS && tid == 0 && t < F[g]) ops.Mrow[(size_t)(b0 + g) * T + t] = top[g];
                sum[g] = 0.f;
            }
            for (int j = tid; j < S; j += kThreads)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (t >= F[g]) continue;
                    const float la = cur[g * stride + j] - top[g];
                    cur[g * stride + j] = la;
                    post[((size_t)(b0 + g) * T + t) * S + j] = la;
                    if (OPS) ops.LAop[((size_t)(b0 + g) * T + t) * p.S4 + j] = la;
                    sum[g] += ex2(la);
                }
            to_waves<G, false>(tile, 1, sum);
            barrier();
            from_waves<G, false>(tile, 1, sum);                                  // (a butterfly: every lane takes part)
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (tid == 0 && t == F[g] - 1) tile.Zlast[g] = sum[g];
        }
    }

    // ---- L = ln 2 (sum M_t + log2 Z_{F-1}); NaN when that is NaN or +inf, or the promise is broken ----
    if (tid == 0) {
        const bool broken = *flag != 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const double L = (tile.Msum[g] + log2((double)tile.Zlast[g])) * kLn2D;
            const float out = (L != L || L == (double)INFINITY || broken) ? NAN : (float)L;
            tile.L[g] = out;                                                     // (read behind the backward pass's barriers)
            if (b0 + g < B) loglik[b0 + g] = out;
        }
    }
    for (int e = tid; e < G * stride; e += kThreads) rows[e] = -INFINITY;        // (the backward pass puts state x elsewhere)
    barrier();

    // ---- backward: r_t to the row, gamma_t over la_t in place ----
    {
        float *const cur = rows + p.left4[1];
        float *const qrow = tile.smax;                                           // slice 0 of a state, free once it is combined
        for (int t = Fmax - 1; t >= 0; --t) {
            if (t < Fmax - 1) {
                band_phase(tile, p, 1, Pb, S);
                barrier();
            }
            float topq[G], topr[G], outside[G];
            if (t < Fmax - 1) from_waves<G, false>(tile, 1, outside);            // sum_j 2^r_{t+1}[j]
#pragma unroll
            for (int g = 0; g < G; ++g) {
                topq[g] = topr[g] = -INFINITY;
                outside[g] = finite && t < Fmax - 1 ? bg2 + lg2(outside[g]) : 0.f;
            }
            for (int j = tid; j < S; j += kThreads)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (t >= F[g]) continue;
                    const size_t at = ((size_t)(b0 + g) * T + t) * S + j;
                    const float o = obs[at] * kLog2e, la = post[at];
                    const float y = t == F[g] - 1 ? 0.f : product_of(tile, p, g, j, finite, outside[g]);
                    const float q = la + y, r = o + y;
                    qrow[(size_t)g * p.S4 + j] = q;
                    cur[g * stride + j] = r;
                    topq[g] = fb::nan_max(topq[g], q);
                    topr[g] = fb::nan_max(topr[g], r);
                }
            to_waves<G, true>(tile, 2, topq);
            to_waves<G, true>(tile, 3, topr);
            barrier();
            from_waves<G, true>(tile, 2, topq);
            from_waves<G, true>(tile, 3, topr);
            float sumq[G], sumr[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                topq[g] = ref_of(topq[g]);
                topr[g] = ref_of(topr[g]);
                sumq[g] = sumr[g] = 0.f;
            }
            for (int j = tid; j < S; j += kThreads)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (t >= F[g]) continue;
                    const float e = ex2(qrow[(size_t)g * p.S4 + j] - topq[g]);
                    qrow[(size_t)g * p.S4 + j] = e;
                    sumq[g] += e;
                    const float r = cur[g * stride + j] - topr[g];
                    cur[g * stride + j] = r;
                    sumr[g] += ex2(r);
                }
            to_waves<G, false>(tile, 4, sumq);
            to_waves<G, false>(tile, 1, sumr);
            barrier();
            from_waves<G, false>(tile, 4, sumq);
            float shift[OPS ? G : 1];                                            // what turns the row's r into Wop
            if (OPS) {
#pragma unroll
                for (int g = 0; g < G; ++g)
                    shift[g] = t < F[g] ? topr[g] - (ops.Mrow[(size_t)(b0 + g) * T + t] + topq[g] + lg2(sumq[g])) : 0.f;
            }
            for (int j = tid; j < S; j += kThreads)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (t >= F[g]) continue;
                    post[((size_t)(b0 + g) * T + t) * S + j] = isfinite(tile.L[g]) ? qrow[(size_t)g * p.S4 + j] / sumq[g] : NAN;
                    if (OPS) ops.Wop[((size_t)(b0 + g) * T + t) * p.S4 + j] = cur[g * stride + j] + shift[g];
                }
            barrier();                                                           // (phase A writes the slices the line above reads)
        }
    }
}

}  // namespace fbl
