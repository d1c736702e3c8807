// forward_backward_wide_band.hpp -- state posteriors and log-likelihood for a transition matrix that holds ONE value outside
// a band of up to 512 entries (torbi_hip_forward_backward_wide_band, torbi_amd/posterior.py forward_backward_wide_banded,
// POSTERIOR.md "Wide band route").
//
// The model, the contract, the scaled recurrence, the band split (E - ebg over the band plus ebg * c_{t-1}, backward
// ebg * sum w_{t+1}), the promise flag and the non-finite rules are forward_backward_band.hpp's; so are the launches: pack
// (with the flag reset), verify, row maxima, then ONE launch that runs every frame of both passes, a workgroup of 1024
// threads owning G whole items.  New is how a frame's band sum is done: the sum-product sibling of band_tile_forward.hpp's
// register tile, where fb_band_kernel issues one 4-byte LDS read and one 4-byte L2 load per G multiply-adds.
//
// A pass sees the band from its output state x: forward x is the next state and looks `left` = reach_left back, backward x
// is the prev state and looks `left` = reach_right back.  With left4 = `left` rounded up to 4 and shift = left4 - left, the
// diagonal d (0 <= d < W + shift) of output x reads input x - left4 + d; the `shift` leading diagonals are zero.  They make
// every 16-byte piece of the LDS row window aligned.
//
// Pack (once per call, one per pass, in the order the lanes read it; clipped positions are 0, ebg is subtracted):
//     P [256-state block b][dquad q][diagonal c of the quad][lane l][4 states]     4 KiB per (block, dquad)
//     P[b][q][c][l][n] = E(output x = 256 b + 4 l + n, diagonal 4 q + c) - ebg
// so every load instruction of a wave is one contiguous KiB.  1.08 MB a pass at 1440 states and 175 diagonals.
//
// A frame of a pass takes two phases and two barriers:
//   A  band sum.  Wave w < blocks * slices owns block w % blocks and slice w / blocks of the dquads; a lane owns 4
//      consecutive states x the G items of the tile.  Per dquad it loads 4 x 16 B of band (global_load_dwordx4, one or two
//      dquads in flight) and per item ONE new 16-byte piece of the row window (the upper half of the last one is kept), for
//      16 G multiply-adds: out[n] += P[c][n] * window[n + c].  The slice's sums go to LDS, part [slice][G][S].
//   B  a thread per state (tid, tid + 1024, ...), as in fb_band_kernel: the slices of a state are added in slice order, then
//      the observation, the scaling and the outputs; the row is written in place (every reader is behind the barrier).
// The observations (and a_t backward) of the first states of a thread are asked for before phase A.
//
// LDS of a tile: rows [G][stride] with stride = S4 + 4 Dq + 4 (state x of the pass at `left4 + x`, zeros elsewhere), the
// slices [KS][G][S4], the wave sums of a row [2][G][16] and fb_band_kernel's fp64 sums of L.
//
// The order of every sum of an item is fixed by (S, band) alone: dquads ascending and diagonals ascending within a slice,
// slices ascending, then fb_band_kernel's butterflies.  An item's bits depend neither on G nor on its tile nor on the batch.
// No float atomics, vector stores only, nothing waits across workgroups.
//
// The body of the launch is wide_passes<G, COUNTS>.  fb_wide_band_kernel<G> is its `false` arm.  The `true` arm,
// fb_wide_band_operands_kernel<G>, also leaves the two factors of every pair of the expected counts in the workspace
// (counts_wide_band.hpp); it is a second kernel, by counts_band.hpp's reasoning: the posterior route keeps its instances.
// The forward pass is wide_forward<G>, which fb_wide_band_filter_kernel<G> (sample_wide_band.hpp) runs alone.
#pragma once

#include "forward_backward_band.hpp"

namespace fbw {

constexpr int kThreads = fbb::kThreads, kWaves = fbb::kWaves;
constexpr int kMaxStates = 4096;
constexpr int kMaxWindow = 512;              // in-band entries of one matrix row, after clamping the reaches to S - 1
constexpr int kMaxGroup = 4;                 // items per workgroup (8 needs scratch within the 128 VGPRs of a lane at 16 waves)
constexpr int kMaxLdsBytes = 160 * 1024;     // the LDS of a compute unit
constexpr int kBlockStates = 256;            // states of a wave: 64 lanes x 4

// The kernels of this file are built with packed fp32 instructions off (v_pk_fma_f32 and its kin): every multiply-add is one
// scalar fmaf.  Under the build's -fno-slp-vectorize the compiler emits no packed form with or without the attribute, so it
// changes no instruction today; a float2 fmaf over pairs of items is open work and would lift it.  What the attribute costs:
// a function of the default target is inlined into these kernels only when it is forced, so everything they use is
// __forceinline__ or always_inline, the barrier is spelled out below, and 16-byte pieces are the native vector type f4, not
// HIP's float4 with its out-of-line constructors.  profiles/posterior_wide_band_kernel_registers.txt counts the calls in the
// ISA: none.
#if defined(__HIP_DEVICE_COMPILE__)
#define FBW_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#define FBW_INLINE __device__ __forceinline__ __attribute__((target("no-packed-fp32-ops")))
#else
#define FBW_KERNEL __global__
#define FBW_INLINE __device__ __forceinline__
#endif

// (__syncthreads, spelled out: a function of another target is not inlined into these kernels unless it is forced)
__device__ __forceinline__ void barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

typedef float f4 __attribute__((ext_vector_type(4)));     // one 16-byte piece

__host__ __device__ inline int up4(int x) { return (x + 3) & ~3; }

// what the band is to the kernel.  Pass 0 is forward, pass 1 backward.
struct Plan {
    int reach_left, reach_right, W;
    int S4, blocks, slices;                  // S up to 4; 256-state blocks; slices of the dquads (blocks * slices <= 16 waves)
    int left[2], left4[2], Dq[2];            // per pass: reach towards lower states, the same up to 4, dquads
    int stride;                              // floats of one LDS row
};
__host__ __device__ inline Plan plan_of(int S, int reach_left, int reach_right) {
    Plan p;
    p.reach_left = fbb::clamp_reach(reach_left, S);
    p.reach_right = fbb::clamp_reach(reach_right, S);
    p.W = p.reach_left + p.reach_right + 1;
    p.S4 = up4(S);
    p.blocks = (p.S4 + kBlockStates - 1) / kBlockStates;
    p.left[0] = p.reach_left;
    p.left[1] = p.reach_right;
    for (int pass = 0; pass < 2; ++pass) {
        p.left4[pass] = up4(p.left[pass]);
        p.Dq[pass] = (p.W + p.left4[pass] - p.left[pass] + 3) / 4;
    }
    const int least = p.Dq[0] < p.Dq[1] ? p.Dq[0] : p.Dq[1], most = p.Dq[0] > p.Dq[1] ? p.Dq[0] : p.Dq[1];
    p.slices = kWaves / p.blocks;
    p.slices = p.slices > least ? least : p.slices;
    p.stride = p.S4 + 4 * most + 4;          // (the last lane with a state reads up to S4 - 4 + 4 (most - 1) + 7; lanes past S read nothing)
    return p;
}
__host__ __device__ inline size_t pack_floats(const Plan &p, int pass) { return (size_t)p.blocks * p.Dq[pass] * 1024; }

struct Layout : Plan { float *P[2], *m, *c; int32_t *flag; size_t total; };

// `base`: the caller's workspace aligned up to 256 bytes, or null for the byte count alone
inline Layout layout(char *base, int B, int T, int S, int reach_left, int reach_right) {
    Layout l;
    static_cast<Plan &>(l) = plan_of(S, reach_left, reach_right);
    Scratch a(base);
    l.P[0] = a.take<float>(pack_floats(l, 0));
    l.P[1] = a.take<float>(pack_floats(l, 1));
    l.m = a.take<float>((size_t)B * T);
    l.c = a.take<float>((size_t)B * T);
    l.flag = a.take<int32_t>(1);
    l.total = a.bytes + 256;                 // (room to align the caller's base)
    return l;
}

// LDS of a tile of G items, in this order: fp64 wave sums of L [G][16] and L [G]; rows [G][stride]; slices [KS][G][S4]; wave
// sums of a row [2][G][16]
__host__ __device__ inline size_t rows_offset(int G) { return ((size_t)G * (kWaves + 1) * 8 + 15) & ~(size_t)15; }
__host__ __device__ inline size_t lds_bytes(int G, const Plan &p) {
    return rows_offset(G) + (size_t)G * 4 * ((size_t)p.stride + (size_t)p.slices * p.S4 + 2 * kWaves);
}

// ---- both packs of E - ebg; resets the promise flag.  grid (blocks * max Dq, 2 passes), block 256 = 4 diagonals x 64 lanes ----
FBW_KERNEL __launch_bounds__(256) void fb_wide_pack_kernel(const float *__restrict__ A, float *__restrict__ Pf,
                                                            float *__restrict__ Pb, int32_t *__restrict__ flag, float ebg,
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
        v[n] = in ? expf(A[at]) - ebg : 0.f;
    }
    f4 *out = reinterpret_cast<f4 *>(pass == 0 ? Pf : Pb);
    out[(((size_t)blk * Dq + q) * 4 + c) * 64 + lane] = f4{v[0], v[1], v[2], v[3]};
}

// host: the pack, then fb_band_verify_kernel's check of the promise
inline hipError_t pack_and_verify(const float *A, const Layout &l, float ebg, float background, int S, hipStream_t st) {
    const int most = l.Dq[0] > l.Dq[1] ? l.Dq[0] : l.Dq[1];
    hipLaunchKernelGGL(fb_wide_pack_kernel, dim3((unsigned)(l.blocks * most), 2), dim3(256), 0, st, A, l.P[0], l.P[1], l.flag, ebg,
                       static_cast<const Plan &>(l), S);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fbb::fb_band_verify_kernel, dim3(S), dim3(64), 0, st, A, l.flag, background, l.reach_left, l.reach_right, S);
    return hipGetLastError();
}

// dquads of band a lane holds in registers: the one it multiplies and those in flight behind it
constexpr int band_buffers(int G) { return G <= 2 ? 3 : 2; }
// phase-B states of a thread whose observation (and a_t) is asked for before phase A
constexpr int early_states(int G) { return G <= 2 ? 2 : 0; }

// One tile: fb_band_kernel's, with this kernel's LDS (rows: ONE per item, written in place)
template <int G>
struct Tile : fbb::Tile<G> {
    float *slice;                            // [KS][G][S4]
    __device__ __forceinline__ Tile(unsigned char *lds, const Plan &p, int S) : fbb::Tile<G>(lds, 0, 0, S) {
        this->lsum = reinterpret_cast<double *>(lds);
        this->Ls = this->lsum + G * kWaves;
        this->rows = reinterpret_cast<float *>(lds + rows_offset(G));
        this->stride = p.stride;
        slice = this->rows + (size_t)G * p.stride;
        this->part = slice + (size_t)p.slices * G * p.S4;
    }
};

// ---- phase A of one lane: acc[g][n] = sum over the dquads [q_lo, q_hi) of P[q][c][n] * row_g[4 q + c + n] ----
// `pack`: the lane's first piece of its block (piece (q, c) 64 (4 q + c) f4 on); `row`: item 0's row at the lane's
// first state (item g: g * stride floats on).  q_lo < q_hi, both the same in every lane of the wave.
template <int G>
__device__ __forceinline__ void band_sum(const f4 *__restrict__ pack, const float *row, int stride, int q_lo, int q_hi,
                                         float (&acc)[G][4]) {
    constexpr int D = band_buffers(G);
    f4 buf[D][4];
#pragma unroll
    for (int u = 0; u < D - 1; ++u) {
        const int q = q_lo + u < q_hi ? q_lo + u : q_hi - 1;             // (past the slice: its last dquad again)
#pragma unroll
        for (int c = 0; c < 4; ++c) buf[u][c] = pack[(size_t)(4 * q + c) * 64];
    }
    f4 lo[G];
#pragma unroll
    for (int g = 0; g < G; ++g) lo[g] = *reinterpret_cast<const f4 *>(row + g * stride + 4 * q_lo);
    for (int q0 = q_lo; q0 < q_hi; q0 += D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int q = q0 + u;
            if (q < q_hi) {
                const int qn = q + D - 1 < q_hi ? q + D - 1 : q_hi - 1;
#pragma unroll
                for (int c = 0; c < 4; ++c) buf[(u + D - 1) % D][c] = pack[(size_t)(4 * qn + c) * 64];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const f4 hi = *reinterpret_cast<const f4 *>(row + g * stride + 4 * q + 4);
                    const float v[8] = {lo[g].x, lo[g].y, lo[g].z, lo[g].w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float d[4] = {buf[u][c].x, buf[u][c].y, buf[u][c].z, buf[u][c].w};
#pragma unroll
                        for (int n = 0; n < 4; ++n) acc[g][n] = fmaf(d[n], v[n + c], acc[g][n]);
                    }
                    lo[g] = hi;
                }
            }
        }
    }
}

// phase A of the workgroup for one pass: every owning wave's slice sums to tile.slice (the caller's barrier follows)
template <int G>
__device__ __forceinline__ void band_phase(const Tile<G> &tile, const Plan &p, int pass, const float *__restrict__ P, int S) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave >= p.blocks * p.slices) return;
    const int blk = wave % p.blocks, sl = wave / p.blocks, Dq = p.Dq[pass];
    const int per = (Dq + p.slices - 1) / p.slices;
    const int q_lo = sl * per, q_hi = q_lo + per < Dq ? q_lo + per : Dq;
    const int x0 = kBlockStates * blk + 4 * lane;
    if (x0 >= S) return;
    float acc[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[g][n] = 0.f;
    if (q_lo < q_hi)
        band_sum<G>(reinterpret_cast<const f4 *>(P) + (size_t)blk * Dq * 256 + lane, tile.rows + x0, tile.stride, q_lo, q_hi, acc);
#pragma unroll
    for (int g = 0; g < G; ++g)
        *reinterpret_cast<f4 *>(tile.slice + ((size_t)sl * G + g) * p.S4 + x0) = f4{acc[g][0], acc[g][1], acc[g][2], acc[g][3]};
}

// the band sum of state j of item g: the slices in their order
template <int G>
__device__ __forceinline__ float slices_of(const Tile<G> &tile, int S4, int KS, int g, int j) {
    float s = tile.slice[(size_t)g * S4 + j];
    for (int k = 1; k < KS; ++k) s += tile.slice[((size_t)k * G + g) * S4 + j];
    return s;
}

// items b0 .. b0 + G - 1 of the workgroup: their frames, and zero rows (no barrier: the caller's next one covers the rows)
template <int G>
__device__ __forceinline__ void tile_begin(Tile<G> &tile, const int32_t *__restrict__ frames, int B, int T) {
    tile.b0 = blockIdx.x * G;
    tile.Fmax = 1;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        tile.F[g] = tile.b0 + g < B ? fb::frames_of(frames, tile.b0 + g, T) : 0;    // (0: an item beyond the batch never takes a step)
        tile.Fmax = tile.F[g] > tile.Fmax ? tile.F[g] : tile.Fmax;
    }
    for (int e = threadIdx.x; e < G * tile.stride; e += kThreads) tile.rows[e] = 0.f;
}

// ---- forward: a_0 = exp(pi + o_0 - m_0), a_t = e_t * (E a_{t-1}) / c_{t-1}; a_t to `out` (rows of `out_stride` floats), c_t
// to cbuf; ends behind a barrier, with every c_t of the tile stored.  The one forward pass of fb_wide_band_kernel,
// fb_wide_band_operands_kernel and fb_wide_band_filter_kernel (sample_wide_band.hpp): it fixes the bits of a_t, c_t and L ----
template <int G>
FBW_INLINE void wide_forward(const Tile<G> &tile, const float *__restrict__ obs, const float *__restrict__ initial,
                             const float *__restrict__ Pf, const float *__restrict__ m, float *__restrict__ cbuf,
                             float *__restrict__ out, int out_stride, float ebg, const Plan &p, int T, int S) {
    constexpr int kEarly = early_states(G);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stride = p.stride, S4 = p.S4, KS = p.slices, b0 = tile.b0;
    const int *F = tile.F;
    const int Fmax = tile.Fmax;
    float *const part = tile.part;
    float *const cur = tile.rows + p.left4[0];
    for (int t = 0; t < Fmax; ++t) {
        float mt[G], early[kEarly > 0 ? kEarly : 1][G];
        auto scalars = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int g = 0; g < G; ++g) mt[g] = t < F[g] ? m[(size_t)(b0 + g) * T + t] : 0.f;
        };
        if (kEarly > 0) scalars();                                   // (a large tile has no registers to hold them over phase A)
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int it = 0; it < kEarly; ++it) {
                const int j = tid + it * kThreads;
                early[it][g] = (j < S && t < F[g]) ? obs[((size_t)(b0 + g) * T + t) * S + j] : 0.f;
            }
        if (t > 0) {
            band_phase(tile, p, 0, Pf, S);
            barrier();
        }
        if (kEarly == 0) scalars();
        float cprev[G], acc[G];
        if (t > 0) fbb::row_sums(tile, t - 1, cbuf, T, cprev);
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = 0.f;
        auto state = [&](int j, const float *ot) __attribute__((always_inline)) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t >= F[g]) continue;
                const size_t row = (size_t)(b0 + g) * T + t;
                const float o = ot ? ot[g] : obs[row * S + j], mm = mt[g];
                float v;
                if (t == 0) {
                    v = expf(initial[j] + o - mm);
                } else {
                    const float s = slices_of(tile, S4, KS, g, j);
                    const float e = expf(o - mm), c = cprev[g];
                    const float u = e * (ebg != 0.f ? fmaf(ebg, c, s) : s);
                    v = c == 0.f ? u * 0.f : u / c;                  // (after a zero-probability frame: 0, or NaN from NaN)
                }
                cur[g * stride + j] = v;
                out[row * out_stride + j] = v;
                acc[g] += v;
            }
        };
#pragma unroll
        for (int it = 0; it < kEarly; ++it)
            if (tid + it * kThreads < S) state(tid + it * kThreads, early[it]);
        for (int j = tid + kEarly * kThreads; j < S; j += kThreads) state(j, nullptr);
        float *w = part + (size_t)(t & 1) * G * kWaves;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float a = fbb::wave_sum(acc[g]);
            if (lane == 0) w[g * kWaves + wave] = a;
        }
        barrier();
    }
    float c[G];
    fbb::row_sums(tile, Fmax - 1, cbuf, T, c);
    barrier();                                                     // (c_t written by thread 0 is read by all below)
}

// ---- both passes of G items of one workgroup, the body of the two kernels below.  COUNTS (counts_wide_band.hpp): backward
// phase B also stores the two operand rows of the counts, Wop[b][t][j] = w_t[j] and Aop[b][t][j] = a_t[j] * (g_b / c_t), rows
// of S4 floats; `false` is the posterior kernel as it was, and nothing of `true` touches a value `false` computes ----
template <int G, bool COUNTS>
FBW_INLINE void wide_passes(unsigned char *lds_raw, const float *__restrict__ obs, const int32_t *__restrict__ frames,
                            const float *__restrict__ initial, const float *__restrict__ Pf, const float *__restrict__ Pb,
                            const float *__restrict__ m, float *__restrict__ cbuf, const int32_t *__restrict__ flag,
                            const float *__restrict__ weights, float *__restrict__ post, float *__restrict__ loglik,
                            float *__restrict__ Wop, float *__restrict__ Aop, float ebg, const Plan &p, int B, int T, int S) {
    constexpr int kEarly = early_states(G);
    Tile<G> tile(lds_raw, p, S);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stride = p.stride, S4 = p.S4, KS = p.slices;
    tile_begin(tile, frames, B, T);
    const int b0 = tile.b0;
    const int *F = tile.F;
    const int Fmax = tile.Fmax;
    float *const rows = tile.rows, *const part = tile.part;
    fbb::zero_absent_rows(tile, post, B, T, S);
    barrier();

    wide_forward(tile, obs, initial, Pf, m, cbuf, post, S, ebg, p, T, S);
    fbb::log_likelihood(tile, m, cbuf, flag, loglik, B, T);
    for (int e = tid; e < G * stride; e += kThreads) rows[e] = 0.f;      // (the backward pass puts state x elsewhere)
    barrier();

    // ---- backward: b_{F-1} = 1, b_t = E^T w_{t+1}; gamma_t = a_t b_t / c_t in place, w_t = e_t b_t / c_t ----
    float *const cur = rows + p.left4[1];
    for (int t = Fmax - 1; t >= 0; --t) {
        const bool step = t < Fmax - 1;
        float mt[G], ct[G], gc[COUNTS ? G : 1], early_o[kEarly > 0 ? kEarly : 1][G], early_a[kEarly > 0 ? kEarly : 1][G];
        auto scalars = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                mt[g] = t < F[g] ? m[(size_t)(b0 + g) * T + t] : 0.f;
                ct[g] = t < F[g] ? cbuf[(size_t)(b0 + g) * T + t] : 1.f;
                if (COUNTS) gc[g] = (weights && b0 + g < B ? weights[b0 + g] : 1.f) / ct[g];
            }
        };
        if (kEarly > 0) scalars();
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int it = 0; it < kEarly; ++it) {
                const int j = tid + it * kThreads;
                const size_t at_j = ((size_t)(b0 + g) * T + t) * S + j;
                early_o[it][g] = (j < S && t < F[g]) ? obs[at_j] : 0.f;
                early_a[it][g] = (j < S && t < F[g]) ? post[at_j] : 0.f;
            }
        if (step) {
            band_phase(tile, p, 1, Pb, S);
            barrier();
        }
        if (kEarly == 0) scalars();
        float sw[G], acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) sw[g] = acc[g] = 0.f;
        if (ebg != 0.f && step) {
            const float *w = part + (size_t)((t & 1) ^ 1) * G * kWaves;
#pragma unroll
            for (int g = 0; g < G; ++g) sw[g] = fbb::sum16(w[g * kWaves + (lane & 15)]);
        }
        auto state = [&](int j, const float *ot, const float *at) __attribute__((always_inline)) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (t >= F[g]) continue;
                const size_t at_j = ((size_t)(b0 + g) * T + t) * S + j;
                const float o = ot ? ot[g] : obs[at_j], a = at ? at[g] : post[at_j], mm = mt[g], c = ct[g];
                float beta = 1.f;
                if (t != F[g] - 1) {
                    const float s = slices_of(tile, S4, KS, g, j);
                    beta = ebg != 0.f ? fmaf(ebg, sw[g], s) : s;
                }
                const float w = (expf(o - mm) * beta) / c;               // (w_0 is never read)
                post[at_j] = isfinite(tile.Ls[g]) ? (a * beta) / c : NAN;
                if (COUNTS) {
                    const size_t at_c = ((size_t)(b0 + g) * T + t) * S4 + j;
                    Wop[at_c] = w;
                    Aop[at_c] = a * gc[g];
                }
                cur[g * stride + j] = w;
                acc[g] += w;
            }
        };
#pragma unroll
        for (int it = 0; it < kEarly; ++it)
            if (tid + it * kThreads < S) state(tid + it * kThreads, early_o[it], early_a[it]);
        for (int j = tid + kEarly * kThreads; j < S; j += kThreads) state(j, nullptr, nullptr);
        if (ebg != 0.f) {
            float *w = part + (size_t)(t & 1) * G * kWaves;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float a = fbb::wave_sum(acc[g]);
                if (lane == 0) w[g * kWaves + wave] = a;
            }
        }
        barrier();
    }
}

// ---- the posteriors: grid ceil(B / G), dynamic LDS lds_bytes(G, plan) ----
template <int G>
FBW_KERNEL __launch_bounds__(kThreads) void fb_wide_band_kernel(const float *__restrict__ obs, const int32_t *__restrict__ frames,
                                                                const float *__restrict__ initial, const float *__restrict__ Pf,
                                                                const float *__restrict__ Pb, const float *__restrict__ m,
                                                                float *__restrict__ cbuf, const int32_t *__restrict__ flag,
                                                                float *__restrict__ post, float *__restrict__ loglik, float ebg,
                                                                Plan p, int B, int T, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    wide_passes<G, false>(lds_raw, obs, frames, initial, Pf, Pb, m, cbuf, flag, nullptr, post, loglik, nullptr, nullptr, ebg, p, B,
                          T, S);
}

// ---- the posteriors and the operand rows of the counts: the same grid and LDS ----
template <int G>
FBW_KERNEL __launch_bounds__(kThreads) void fb_wide_band_operands_kernel(
    const float *__restrict__ obs, const int32_t *__restrict__ frames, const float *__restrict__ initial,
    const float *__restrict__ Pf, const float *__restrict__ Pb, const float *__restrict__ m, float *__restrict__ cbuf,
    const int32_t *__restrict__ flag, const float *__restrict__ weights, float *__restrict__ post, float *__restrict__ loglik,
    float *__restrict__ Wop, float *__restrict__ Aop, float ebg, Plan p, int B, int T, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    wide_passes<G, true>(lds_raw, obs, frames, initial, Pf, Pb, m, cbuf, flag, weights, post, loglik, Wop, Aop, ebg, p, B, T, S);
}

#undef FBW_KERNEL
#undef FBW_INLINE

}  // namespace fbw
